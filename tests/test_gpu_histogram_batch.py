"""GPU tests of the batched histogram (glu_histogram_run_batch_even_ptr, _batch_offsets_even_ptr, _batch_edges_ptr,
_batch_offsets_edges_ptr): out_counts[s * bins + b] = the samples of segment s in bin b.  The oracle is numpy's restatement of the single
call's contract, applied to each segment's slice (the bin of every sample by the rule, then one bincount over segment * bins + bin),
and every comparison is `==`:
  even integers  (x.astype(int64) - lo) // W
  even floats    minimum(((x.astype(float64) - lo) * scale).astype(int64), bins - 1), NaN dropped
  edges          searchsorted(edges, x, side="right") - 1, NaN samples removed
Every array a call writes sits inside an allocation with 64 bytes of poison in front of it and behind it and is itself filled with
poison first; the inputs are checked unchanged; read_batch() is checked against plan_histogram_batch and last() against the kernels
the header states.  Sizes come from plan_histogram_batch.  The scheme is that of test_gpu_histogram.py."""
import gc
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
POISON = 0xA5
POISON32 = 0xA5A5A5A5
BATCH = 2  # HistogramPath_Batch
GIB = 1 << 30


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert built.HistogramPath_Batch == BATCH
    return built


class Array:
    """The bytes of `d` on the device, `shift` bytes behind a 16-byte boundary, between GUARD bytes of poison."""

    def __init__(self, d, shift=0):
        import torch

        d = np.ascontiguousarray(d)
        self.dtype, self.nbytes, self.front = d.dtype, d.nbytes, GUARD + shift
        host = np.concatenate([np.full(self.front, POISON, dtype=np.uint8), d.view(np.uint8).ravel(), np.full(GUARD, POISON, dtype=np.uint8)])
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.front

    @classmethod
    def poisoned(cls, nbytes, shift=0):
        return cls(np.full(nbytes, POISON, dtype=np.uint8), shift)

    def result(self, dtype=None):
        raw = self.t.cpu().numpy()
        assert (raw[:self.front] == POISON).all() and (raw[self.front + self.nbytes:] == POISON).all(), "the call wrote outside the array"
        return raw[self.front:self.front + self.nbytes].copy().view(dtype or self.dtype)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def even_bins_of(x, lo, hi, bins):
    """The bin of every sample by the contract's restatement, -1 where it is not counted."""
    if x.dtype.kind == "f":
        d = x.astype(np.float64)
        flo, fhi = np.float64(lo), np.float64(hi)
        scale = np.float64(bins) / (fhi - flo)
        inside = (d >= flo) & (d < fhi)
        with np.errstate(invalid="ignore"):
            b = np.minimum(((np.where(inside, d, flo) - flo) * scale).astype(np.int64), bins - 1)
    else:
        w, rem = divmod(int(hi) - int(lo), bins)
        assert rem == 0 and w >= 1
        wide = x.astype(np.int64)
        inside = (wide >= lo) & (wide < hi)
        b = (wide - int(lo)) // w
    return np.where(inside, b, -1)


def edges_bins_of(x, e):
    bins = e.size - 1
    b = np.searchsorted(e, x, side="right").astype(np.int64) - 1
    if x.dtype.kind == "f":
        b = np.where(np.isnan(x), -1, b)
    return np.where((b >= 0) & (b < bins), b, -1)


def want_rows(bin_of, offsets, bins):
    """Rows of the segments [offsets[s], offsets[s + 1]) (well-formed) from the bin of every sample."""
    offsets = np.asarray(offsets, dtype=np.int64)
    S = offsets.size - 1
    seg = np.repeat(np.arange(S, dtype=np.int64), np.diff(offsets))
    b = bin_of[offsets[0]:offsets[-1]]
    keep = b >= 0
    return np.bincount(seg[keep] * bins + b[keep], minlength=S * bins).astype(np.uint32).reshape(S, bins)


def limits(G, bins, key_type, mode):
    _, _, (wave_limit, block_limit), chunk, row_bytes = G.plan_histogram_batch(1, bins, key_type, mode)
    assert row_bytes == 4 * bins and block_limit == chunk
    return wave_limit, block_limit, chunk


def classes_of(G, lens, bins, key_type, mode):
    out = {"wave": 0, "block": 0, "long": 0}
    for n in np.unique(lens):
        path = G.plan_histogram_batch(int(n), bins, key_type, mode)[0]
        if path:
            out[("wave", "block", "long")[path - 1]] += int((lens == n).sum())
    return out


def kernels_of(G, form, lens, total, bins, key_type, mode, accumulate):
    """The kernels the header states for a call."""
    wave_limit, block_limit, _ = limits(G, bins, key_type, mode)
    S = len(lens)
    if form == "equal":
        path = G.plan_histogram_batch(int(lens[0]), bins, key_type, mode)[0]
        return (0 if accumulate else 1, 1, 1, 2)[path]
    if total == 0:
        return 1
    wave = 1 if wave_limit and min(S, total) else 0
    block = 1 if min(S, total // (wave_limit + 1)) else 0
    long = 2 if min(S, total // (block_limit + 1)) else 0
    return 1 + wave + block + long


def check_batch(G, h, x, offsets, bins, even=None, edges=None, form="offsets", shift=0, out_shift=0, prior=None, well_formed=True, front=0):
    """One batched call over the segments `offsets` (S + 1 values; form "equal": they are s * count) of x on poisoned counts (prior
    None) or on `prior` (accumulate).  `front`: samples of x in front of the array the call is given are not part of it."""
    import torch

    key_type = str(x.dtype)
    mode = "even" if even is not None else "edges"
    offsets = np.asarray(offsets, dtype=np.uint32)
    S = offsets.size - 1
    total = x.size
    xa = Array(bits(x), shift)
    fa = Array(offsets) if form == "offsets" else None
    ea = Array(bits(edges)) if edges is not None else None
    out = Array.poisoned(4 * bins * S, out_shift) if prior is None else Array(prior, out_shift)
    assert xa.ptr % 16 == shift and out.ptr % 16 == out_shift
    sp = xa.ptr if total else None
    if form == "equal":
        count = int(offsets[1]) if S else 0
        assert (np.diff(offsets.astype(np.int64)) == count).all() and count * S == total
        if mode == "even":
            h.run_batch_even_ptr(sp, count, S, even[0], even[1], bins, out.ptr, key_type, prior is not None, stream())
        else:
            h.run_batch_edges_ptr(sp, count, S, ea.ptr, bins, out.ptr, key_type, prior is not None, stream())
    elif mode == "even":
        h.run_batch_offsets_even_ptr(sp, total, fa.ptr, S, even[0], even[1], bins, out.ptr, key_type, prior is not None, stream())
    else:
        h.run_batch_offsets_edges_ptr(sp, total, fa.ptr, S, ea.ptr, bins, out.ptr, key_type, prior is not None, stream())
    torch.cuda.synchronize()
    got = out.result(np.uint32).reshape(S, bins)
    assert (xa.result() == bits(x)).all(), "the call wrote to its samples"
    if fa is not None:
        assert (fa.result() == offsets).all(), "the call wrote to its offsets"
    if ea is not None:
        assert (ea.result() == bits(edges)).all(), "the call wrote to its edges"
    if not well_formed:
        return got
    what = (mode, form, key_type, total, S, bins, shift, out_shift)
    lens = np.diff(offsets.astype(np.int64))
    if S:
        assert h.last() == (BATCH, 0, kernels_of(G, form, lens, total, bins, key_type, mode, prior is not None)), (what, h.last())
        assert h.read_batch() == classes_of(G, lens, bins, key_type, mode), (what, h.read_batch())
    bin_of = even_bins_of(x, even[0], even[1], bins) if mode == "even" else edges_bins_of(x, edges)
    want = want_rows(bin_of, offsets, bins)
    if prior is not None:
        want = want + np.asarray(prior, dtype=np.uint32).reshape(S, bins)  # (modulo 2^32)
        untouched = np.flatnonzero(lens == 0)
        assert (got[untouched] == np.asarray(prior).reshape(S, bins)[untouched]).all(), "the row of an empty segment was touched"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), int(lens[bad[0][0]]))
    return got


def offsets_of(lens, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) + first).astype(np.uint32)


def samples_of(rng, n, key_type, lo, hi):
    """n samples of the type spread over [lo - 10 %, hi + 10 %) of the range"""
    dtype = np.dtype(key_type)
    span = float(hi) - float(lo)
    v = rng.random(n) * span * 1.2 + float(lo) - 0.1 * span
    if dtype.kind != "f":
        info = np.iinfo(dtype)
        v = np.clip(np.floor(v), info.min, info.max)
    return v.astype(dtype)


def class_lengths(G, rng, bins, key_type, mode):
    """The lengths of the issue's class batch in shuffled order, empty segments first, last and in runs."""
    wave_limit, block_limit, chunk = limits(G, bins, key_type, mode)
    w = wave_limit if wave_limit else 1024 // np.dtype(key_type).itemsize * 4  # (no wave class: the lengths stay, in the block class)
    lens = [0, 1, 63, 64, 65, w - 1, w, w + 1, block_limit - 1, block_limit, block_limit + 1, 2 * chunk, 2 * chunk + 1, 0, 0, 0, 7, 0, 0]
    lens = [int(v) for v in rng.permutation(lens)]
    return np.array([0, 0] + lens + [0], dtype=np.int64)


def edges_of(rng, key_type, bins, lo, hi):
    e = np.sort(samples_of(rng, bins + 1, key_type, lo, hi))
    if bins > 5:
        e[5] = e[4]  # (an empty bin)
    return e


@pytest.mark.parametrize("bins", [640, 1, 2, 63, 64, 65, 2048, 2049, 8192])
def test_every_class_in_one_batch_uint32_even_bins(G, bins):
    rng = np.random.default_rng(31)
    lens = class_lengths(G, rng, bins, "uint32", "even")
    x = samples_of(rng, int(lens.sum()), "uint32", 1000, 1000 + 7 * bins)
    h = G.Histogram()
    check_batch(G, h, x, offsets_of(lens), bins, even=(1000, 1000 + 7 * bins))
    want = classes_of(G, lens, bins, "uint32", "even")
    assert want["long"] == 3 and (want["wave"] == 0) == (bins > 2048) and want["wave"] + want["block"] == 10


@pytest.mark.parametrize("bins", [640, 1, 2, 63, 64, 65, 2048, 2049, 8192])
def test_every_class_in_one_batch_uint64_edges(G, bins):
    rng = np.random.default_rng(32)
    lens = class_lengths(G, rng, bins, "uint64", "edges")
    x = samples_of(rng, int(lens.sum()), "uint64", 1000, 2 ** 40)
    e = edges_of(rng, "uint64", bins, 1000, 2 ** 40)
    x[:min(x.size, e.size)] = e[:x.size]  # (samples exactly on the edges)
    check_batch(G, G.Histogram(), x, offsets_of(lens), bins, edges=e)


def leak_batch(rng, key_type, bins, S=3000):
    """S segments of 0 .. 40 samples; every sample of segment s is the lower edge of bin s % bins: row s holds its length in that one
    entry and zeros elsewhere, or a neighbour leaked."""
    lens = rng.integers(0, 41, S)
    dtype = np.dtype(key_type)
    values = (np.arange(S) % bins).astype(np.int64) * 3 + 100
    x = np.repeat(values, lens).astype(dtype)
    return lens, x, (100, 100 + 3 * bins)


def test_no_leak_between_neighbours_at_every_alignment(G):
    rng = np.random.default_rng(33)
    h = G.Histogram()
    lens, x, rng_even = leak_batch(rng, "uint32", 37)
    for shift, out_shift in ((0, 0), (4, 4), (8, 8), (12, 12), (4, 0), (0, 12)):
        got = check_batch(G, h, x, offsets_of(lens), 37, even=rng_even, shift=shift, out_shift=out_shift)
        assert (got[np.arange(lens.size), np.arange(lens.size) % 37] == lens).all() and int(got.sum()) == int(lens.sum())
    # the offsets begin behind the first sample and end in front of the last: the samples around the batch belong to no row
    check_batch(G, h, np.concatenate([x[:5], x, x[:9]]), offsets_of(lens, first=5), 37, even=rng_even, shift=4)


@pytest.mark.parametrize("key_type", ["float64", "uint64"])
def test_no_leak_between_neighbours_wide_samples(G, key_type):
    rng = np.random.default_rng(34)
    h = G.Histogram()
    lens, x, (lo, hi) = leak_batch(rng, key_type, 37)
    for shift in (0, 8):
        if key_type == "float64":
            check_batch(G, h, x, offsets_of(lens), 37, even=(float(lo), float(hi)), shift=shift, out_shift=shift)
        else:
            e = (np.arange(38, dtype=np.int64) * 3 + 100).astype(np.uint64)
            check_batch(G, h, x, offsets_of(lens), 37, edges=e, shift=shift, out_shift=4)


def test_consecutive_wave_segments_of_one_value_keep_their_adds_apart(G):
    """The HistPending boundary: every sample of every segment is the same value, so a wave holds back one add per segment; carried
    across the boundary it would land in the next row.  Lengths around the packs a wave reads at a time."""
    rng = np.random.default_rng(35)
    wave_limit, _, _ = limits(G, 16, "uint32", "even")
    lens = rng.choice([1, 3, 64, 255, 256, 257, 512, wave_limit - 1, wave_limit], 600)
    x = np.full(int(lens.sum()), 1003, dtype=np.uint32)
    for shift in (0, 4):
        got = check_batch(G, G.Histogram(), x, offsets_of(lens), 16, even=(1000, 1016), shift=shift)
        assert (got[:, 3] == lens).all()
    got = check_batch(G, G.Histogram(), x[:600 * 256], np.arange(601) * 256, 16, even=(1000, 1016), form="equal")
    assert (got[:, 3] == 256).all()


def special_floats(rng, n, dtype):
    x = (rng.random(n) * 6 - 3).astype(dtype)
    x[rng.integers(0, n, n // 7 + 1)] = np.nan
    x[rng.integers(0, n, n // 9 + 1)] = np.inf
    x[rng.integers(0, n, n // 9 + 1)] = -np.inf
    x[rng.integers(0, n, n // 9 + 1)] = 0.0
    x[rng.integers(0, n, n // 9 + 1)] = -0.0
    return x


def typed_lengths(G, bins, key_type, mode):
    wave_limit, block_limit, chunk = limits(G, bins, key_type, mode)
    return np.array([0, 5, wave_limit - 3, 0, wave_limit + 9, block_limit - 1, chunk + 11, 0, 3], dtype=np.int64)  # every class


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32", "float64"])
def test_every_even_type_in_every_class(G, key_type):
    rng = np.random.default_rng(36)
    lens = typed_lengths(G, 100, key_type, "even")
    n = int(lens.sum())
    if key_type in ("float32", "float64"):
        x, even = special_floats(rng, n, np.dtype(key_type)), (-1.5, 2.25)
    else:
        even = (1000, 5000) if key_type == "uint32" else (-3000, 1000)
        x = samples_of(rng, n, key_type, *even)
    check_batch(G, G.Histogram(), x, offsets_of(lens), 100, even=even)


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32", "uint64", "int64", "float64"])
def test_every_edges_type_in_every_class(G, key_type):
    rng = np.random.default_rng(37)
    lens = typed_lengths(G, 33, key_type, "edges")
    n = int(lens.sum())
    dtype = np.dtype(key_type)
    if dtype.kind == "f":
        x = special_floats(rng, n, dtype)
        e = np.sort((rng.random(34) * 5 - 2.5).astype(dtype))
        e[0], e[10], e[11], e[-1] = -np.inf, -0.0, 0.0, np.inf
        e = np.sort(e)
    else:
        lo, hi = (-50000, 50000) if dtype.kind != "u" else (1000, 101000)
        x, e = samples_of(rng, n, key_type, lo, hi), edges_of(rng, key_type, 33, lo, hi)
        x[:34] = e
    check_batch(G, G.Histogram(), x, offsets_of(lens), 33, edges=e)


@pytest.mark.parametrize("parts", [1, 37, 5000])
def test_equal_partitions_give_the_bits_of_the_offsets_form(G, parts):
    rng = np.random.default_rng(38)
    wave_limit, block_limit, chunk = limits(G, 50, "uint32", "even")
    h = G.Histogram()
    counts = [0, 1, wave_limit, block_limit - 5, chunk + 77] if parts <= 37 else [0, 1, 300]
    for count in counts:
        x = samples_of(rng, count * parts, "uint32", 0, 500)
        offsets = np.arange(parts + 1, dtype=np.int64) * count
        equal = check_batch(G, h, x, offsets, 50, even=(0, 500), form="equal")
        assert (equal == check_batch(G, h, x, offsets, 50, even=(0, 500))).all()
    e = np.sort(samples_of(rng, 51, "uint32", 0, 500))
    x = samples_of(rng, 300 * parts, "uint32", 0, 500)
    offsets = np.arange(parts + 1, dtype=np.int64) * 300
    assert (check_batch(G, h, x, offsets, 50, edges=e, form="equal") == check_batch(G, h, x, offsets, 50, edges=e)).all()


@pytest.mark.parametrize("form", ["offsets", "equal"])
def test_accumulate_wraps_and_leaves_the_rows_of_empty_segments(G, form):
    rng = np.random.default_rng(39)
    h = G.Histogram()
    if form == "offsets":
        lens = typed_lengths(G, 20, "uint32", "even")
        batches = [lens]
    else:
        wave_limit, block_limit, chunk = limits(G, 20, "uint32", "even")
        batches = [np.full(9, c) for c in (0, 7, wave_limit + 1, chunk + 3)]
    for lens in batches:
        x = samples_of(rng, int(lens.sum()), "uint32", 0, 200)
        prior = (np.uint32(2 ** 32 - 1) - rng.integers(0, 50, lens.size * 20).astype(np.uint32)).astype(np.uint32)  # (near 2^32: they wrap)
        once = check_batch(G, h, x, offsets_of(lens), 20, even=(0, 200), form=form, prior=prior)
        check_batch(G, h, x, offsets_of(lens), 20, even=(0, 200), form=form, prior=once.ravel())  # run twice


def test_skew_one_value_zipf_and_the_last_of_8192_bins(G):
    rng = np.random.default_rng(40)
    h = G.Histogram()
    _, _, chunk = limits(G, 256, "uint32", "even")
    n = 3 * chunk + 5
    one = np.full(n, 77, dtype=np.uint32)
    zipf = np.minimum(rng.zipf(1.3, n), 255).astype(np.uint32)
    lens = [n, 0, n, 900]
    got = check_batch(G, h, np.concatenate([one, zipf, zipf[:900]]), offsets_of(lens), 256, even=(0, 256))
    assert got[0, 77] == n
    _, _, chunk = limits(G, 8192, "uint32", "even")
    lens = [chunk + 1, 5, chunk - 1]
    got = check_batch(G, h, np.full(sum(lens), 8191, dtype=np.uint32), offsets_of(lens), 8192, even=(0, 8192))
    assert (got[:, 8191] == lens).all()


def test_malformed_offsets_stay_in_bounds_and_spare_the_well_formed_rows(G):
    """Decreasing offsets, offsets beyond `total`, a last offset below the first: the poison around every array stays, the samples are
    unchanged (check_batch), and every segment that is well-formed by itself -- begin <= end <= total -- has its row wherever no list
    overflowed (segments that do not overlap cannot overflow one)."""
    rng = np.random.default_rng(41)
    h = G.Histogram()
    wave_limit, block_limit, chunk = limits(G, 30, "uint32", "even")
    lens = np.array([5, 0, wave_limit, 17, block_limit + 5, 3, 2 * chunk + 1, 0, 40, 9], dtype=np.int64)
    good = offsets_of(lens)
    total = int(good[-1])
    x = samples_of(rng, total, "uint32", 0, 300)
    bin_of = even_bins_of(x, 0, 300, 30)

    def rows_right(offsets, got):
        o = offsets.astype(np.int64)
        for s in range(o.size - 1):
            b, e = o[s], o[s + 1]
            want = want_rows(bin_of, [b, e], 30)[0] if b <= e <= total else np.zeros(30, dtype=np.uint32)
            assert (got[s] == want).all(), (s, b, e)

    beyond = good.copy()
    beyond[6:] += np.uint32(3 * chunk)  # the long segment and all behind it end beyond total: empty
    last_below = good.copy()
    last_below[-1] = 2
    wild = good.copy()
    wild[3], wild[-2] = np.uint32(0xFFFFFFFF), np.uint32(0xFFFFFFF0)
    for bad in (beyond, last_below, wild):  # none of these makes two non-empty segments overlap
        rows_right(bad, check_batch(G, h, x, bad, 30, even=(0, 300), well_formed=False))
    for bad in (good[::-1].copy(), rng.permutation(good).astype(np.uint32), rng.integers(0, 2 ** 32, good.size, dtype=np.uint32),
                np.full(good.size, 0xFFFFFFFF, dtype=np.uint32)):
        got = check_batch(G, h, x, bad, 30, even=(0, 300), well_formed=False)
        if bad is not None and int(np.maximum(np.diff(bad.astype(np.int64)), 0).sum()) <= total:  # (no list can overflow)
            rows_right(bad, got)
    # overlapping long segments that ask for more chunks than the batch has: in bounds, whatever the rows hold
    over = np.array([0, total] * 6, dtype=np.uint32)
    over = np.sort(over)[::-1].copy()
    over[::2], over[1::2] = 0, total
    check_batch(G, h, x, over, 30, even=(0, 300), well_formed=False)


def test_a_prepared_call_is_captured_and_replayed_on_other_contents(G):
    import torch

    rng = np.random.default_rng(42)
    wave_limit, block_limit, chunk = limits(G, 33, "float32", "edges")
    lens = np.array([0, 9, wave_limit, block_limit - 2, chunk + 9, 0, 4], dtype=np.int64)
    total, S = int(lens.sum()), lens.size
    h = G.Histogram()
    h.prepare_batch(total, S, 33)
    xt = torch.zeros(total, dtype=torch.float32, device="cuda")
    ft = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
    et = torch.zeros(34, dtype=torch.float32, device="cuda")
    out = torch.zeros(S * 33, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def call(s):
        h.run_batch_offsets_edges_ptr(xt.data_ptr(), total, ft.data_ptr(), S, et.data_ptr(), 33, out.data_ptr(), "float32", False, s)

    with torch.cuda.stream(side):
        ft.copy_(torch.from_numpy(offsets_of(lens).view(np.int32)))
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):  # (an allocation inside the call would end the capture with an error)
            call(torch.cuda.current_stream().cuda_stream)
        for trial in range(4):  # (the contents are filled and the graph replayed on the stream of the capture, as everywhere in this suite)
            x = (rng.random(total) * 6 - 3).astype(np.float32)
            e = np.sort((rng.random(34) * 5 - 2.5).astype(np.float32))
            offsets = offsets_of(rng.permutation(lens))  # other offsets of the same shape
            xt.copy_(torch.from_numpy(x))
            et.copy_(torch.from_numpy(e))
            ft.copy_(torch.from_numpy(offsets.view(np.int32)))
            out.fill_(-1)
            side.synchronize()
            graph.replay()
            side.synchronize()
            got = out.cpu().numpy().view(np.uint32).reshape(S, 33)
            want = want_rows(edges_bins_of(x, e), offsets, 33)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (trial, offsets.tolist(), bad.tolist(), got[bad].sum(axis=1).tolist(), want[bad].sum(axis=1).tolist())


def test_the_same_batch_gives_the_same_bits_three_times(G):
    rng = np.random.default_rng(43)
    lens = class_lengths(G, rng, 200, "float32", "even")
    x = special_floats(rng, int(lens.sum()), np.float32)
    h = G.Histogram()
    runs = [check_batch(G, h, x, offsets_of(lens), 200, even=(-2.0, 2.0)) for _ in range(3)]
    assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all()


def test_argument_errors_name_the_argument_and_write_nothing(G):
    h = G.Histogram()
    x = Array(np.arange(1000, dtype=np.uint32))
    x64 = Array(np.arange(500, dtype=np.uint64))
    f = Array(np.array([0, 10, 1000], dtype=np.uint32))
    e = Array(np.arange(11, dtype=np.uint32))
    out = Array.poisoned(4 * 8192 * 2)
    S = stream()
    cases = [
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 8193, 8193, out.ptr, "uint32", False, S), "bins must be 1 .. 8192"),
        (lambda: h.run_batch_offsets_edges_ptr(x.ptr, 1000, f.ptr, 2, e.ptr, 8193, out.ptr, "uint32", False, S), "bins must be 1 .. 8192"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 10, 0, out.ptr, "uint32", False, S), "bins must be 1 .. 8192"),
        (lambda: h.run_batch_even_ptr(x64.ptr, 250, 2, 0, 10, 10, out.ptr, "uint64", False, S), "has no even bins"),
        (lambda: h.run_batch_offsets_even_ptr(x64.ptr, 500, f.ptr, 2, 0, 10, 10, out.ptr, "int64", False, S), "has no even bins"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 15, 10, out.ptr, "uint32", False, S), "must be a whole number"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 1.0, 1.0, 10, out.ptr, "float32", False, S), "lo and hi must be finite"),
        (lambda: h.run_batch_even_ptr(x.ptr, 2 ** 31, 2, 0, 10, 10, out.ptr, "uint32", False, S), "fewer than 2^32"),
        (lambda: h.run_batch_offsets_even_ptr(x.ptr, 2 ** 32, f.ptr, 2, 0, 10, 10, out.ptr, "uint32", False, S), "fewer than 2^32"),
        (lambda: h.run_batch_offsets_even_ptr(x.ptr, 1000, f.ptr, 2 ** 24 + 1, 0, 10, 10, out.ptr, "uint32", False, S), "exceeds 2^24"),
        (lambda: h.run_batch_even_ptr(x.ptr, 0, 2 ** 24 + 1, 0, 10, 10, out.ptr, "uint32", False, S), "exceeds 2^24"),
        (lambda: h.run_batch_even_ptr(None, 500, 2, 0, 10, 10, out.ptr, "uint32", False, S), "Invalid samples buffer"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 10, 10, None, "uint32", False, S), "Invalid out_counts buffer"),
        (lambda: h.run_batch_edges_ptr(x.ptr, 500, 2, None, 10, out.ptr, "uint32", False, S), "Invalid edges buffer"),
        (lambda: h.run_batch_offsets_even_ptr(x.ptr, 1000, None, 2, 0, 10, 10, out.ptr, "uint32", False, S), "Invalid offsets array"),
        (lambda: h.run_batch_offsets_even_ptr(x.ptr, 1000, f.ptr + 2, 2, 0, 10, 10, out.ptr, "uint32", False, S), "offsets array is not aligned"),
        (lambda: h.run_batch_even_ptr(x.ptr + 2, 499, 2, 0, 10, 10, out.ptr, "uint32", False, S), "samples is not aligned"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 10, 10, out.ptr + 2, "uint32", False, S), "out_counts is not aligned"),
        (lambda: h.run_batch_even_ptr(x.ptr, 500, 2, 0, 10, 10, x.ptr + 3996, "uint32", False, S), "out_counts overlaps samples"),
        (lambda: h.run_batch_edges_ptr(x.ptr, 500, 2, e.ptr, 10, e.ptr + 40, "uint32", False, S), "out_counts overlaps edges"),
        (lambda: h.run_batch_offsets_even_ptr(x.ptr, 1000, f.ptr, 2, 0, 10, 10, f.ptr + 8, "uint32", False, S), "out_counts overlaps offsets"),
        (lambda: G.check(G.lib().glu_histogram_run_batch_even_ptr(None, None, 5, 2, 0, None, None, 10, None, 0, None)), "histogram"),
        (lambda: G.check(G.lib().glu_histogram_run_batch_even_ptr(h._h, x.ptr, 5, 2, 0, None, None, 10, out.ptr, 0, None)), "lo"),
        (lambda: G.check(G.lib().glu_histogram_run_batch_even_ptr(h._h, x.ptr, 5, 2, 9, None, None, 10, out.ptr, 0, None)), "Invalid key type"),
        (lambda: h.prepare_batch(2 ** 32, 10, 10), "fewer than 2^32"),
        (lambda: h.prepare_batch(1000, 2 ** 24 + 1, 10), "exceeds 2^24"),
        (lambda: h.prepare_batch(1000, 10, 8193), "bins must be 1 .. 8192"),
    ]
    for call, message in cases:
        with pytest.raises(G.GluError) as err:
            call()
        assert err.value.status == G.GLU_ERROR_INVALID_ARGUMENT and message in err.value.message, (message, err.value.message)
    import torch

    torch.cuda.synchronize()
    assert (out.result(np.uint32) == POISON32).all() and (x.result() == np.arange(1000)).all() and (f.result() == [0, 10, 1000]).all()
    # arrays that merely touch are fine, num_segments == 0 does nothing with NULL everywhere, an empty batch needs no samples
    h.run_batch_even_ptr(None, 5, 0, 0, 10, 10, None, "uint32", False, S)
    h.run_batch_offsets_edges_ptr(None, 0, None, 0, None, 10, None, "uint32", False, S)
    zero = Array.poisoned(4 * 20)
    h.run_batch_even_ptr(None, 0, 2, 0, 10, 10, zero.ptr, "uint32", False, S)
    torch.cuda.synchronize()
    assert (zero.result(np.uint32) == 0).all() and h.last() == (BATCH, 0, 1)
    h.run_batch_even_ptr(None, 0, 2, 0, 10, 10, zero.ptr, "uint32", True, S)
    assert h.last() == (BATCH, 0, 0)


def need(nbytes):
    """Skips unless `nbytes` and 10 GiB more (the checks' temporaries) are free: test_gpu_wide_indices.py's guard."""
    import torch

    assert nbytes <= 32 * GIB
    if torch.cuda.mem_get_info()[0] < nbytes + 10 * GIB:
        pytest.skip("needs %d GiB of free HBM" % -(-(nbytes + 10 * GIB) // GIB))


def wide_case(G, key_type, total, offsets, run, bin_of_chunk, bins):
    """`total` hashed samples made on the device, the batch of `offsets` counted by `run`, against torch per segment."""
    import torch

    dtype = torch.int64 if key_type == "uint64" else torch.int32
    raw = torch.empty(total + 32, dtype=dtype, device="cuda")  # (16 poisoned elements in front and behind)
    raw.fill_(-1)
    x = raw[16:16 + total]
    step = 1 << 27
    for lo in range(0, total, step):
        i = torch.arange(lo, min(total, lo + step), dtype=torch.int64, device="cuda")
        hashed = (i * 0x9E3779B1) & 0xFFFFFFFF
        hashed = hashed ^ (hashed >> 15)
        x[lo:lo + i.numel()] = ((hashed << 20) | (i & 0xFFFFF)).to(dtype) if key_type == "uint64" else hashed.to(dtype)
    S = len(offsets) - 1
    ft = torch.tensor(offsets, dtype=torch.int64, device="cuda").to(torch.int32)
    guard = torch.full(((S * bins) + 32,), -1, dtype=torch.int32, device="cuda")
    out = guard[16:16 + S * bins]
    run(x.data_ptr(), ft.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert bool((guard[:16] == -1).all()) and bool((guard[16 + S * bins:] == -1).all()), "the call wrote outside out_counts"
    assert bool((raw[:16] == -1).all()) and bool((raw[16 + total:] == -1).all())
    got = out.cpu().numpy().view(np.uint32).reshape(S, bins)
    for s in range(S):
        want = torch.zeros(bins + 1, dtype=torch.int64, device="cuda")
        for lo in range(offsets[s], offsets[s + 1], step):
            hi = min(offsets[s + 1], lo + step)
            want += torch.bincount(bin_of_chunk(x[lo:hi]), minlength=bins + 1)  # (bin `bins`: not counted)
        assert (got[s] == want[:bins].cpu().numpy().astype(np.uint32)).all(), s


def test_eight_byte_samples_past_4_gib_with_a_segment_across_the_boundary(G):
    import torch

    total = (1 << 29) + 170001  # uint64 samples: 4 GiB and more
    need(8 * total)
    # segment 1 (long) ends below byte 2^32, segment 2 (a workgroup's) lies across it, segment 4 (long) behind it
    offsets = [0, 300, (1 << 29) - 10000, (1 << 29) + 10000, (1 << 29) + 10000, total - 7, total]
    edges = (np.arange(18, dtype=np.uint64) << np.uint64(47)) + np.uint64(12345)  # 17 bins; the samples are below 2^52
    et = torch.from_numpy(edges.view(np.int64)).cuda()
    h = G.Histogram()

    def bin_of(chunk):
        b = torch.searchsorted(et, chunk, right=True) - 1
        return torch.where((b >= 0) & (b < 17), b, torch.full_like(b, 17))

    wide_case(G, "uint64", total, offsets, lambda xp, fp, op: h.run_batch_offsets_edges_ptr(xp, total, fp, 6, et.data_ptr(), 17, op, "uint64",
                                                                                         False, stream()), bin_of, 17)
    want = classes_of(G, np.diff(np.array(offsets, dtype=np.int64)), 17, "uint64", "edges")
    assert h.read_batch() == want and want == {"wave": 2, "block": 1, "long": 2}


def test_four_byte_samples_with_a_segment_across_element_2_31(G):
    import torch

    total = (1 << 31) + 150001  # uint32 samples: 8 GiB
    need(4 * total)
    # segment 1 (long) ends below element 2^31, segment 2 (a workgroup's) lies across it, segment 3 (long) behind it
    offsets = [0, 1000, (1 << 31) - 30000, (1 << 31) + 9000, total - 3, total]
    h = G.Histogram()

    def bin_of(chunk):
        v = chunk.to(torch.int64) & 0xFFFFFFFF
        return torch.where(v < 250 * (1 << 24), v >> 24, torch.full_like(v, 250))

    wide_case(G, "uint32", total, offsets, lambda xp, fp, op: h.run_batch_offsets_even_ptr(xp, total, fp, 5, 0, 250 << 24, 250, op, "uint32", False,
                                                                                        stream()), bin_of, 250)
    want = classes_of(G, np.diff(np.array(offsets, dtype=np.int64)), 250, "uint32", "even")
    assert h.read_batch() == want and want == {"wave": 2, "block": 1, "long": 2}


def test_sort_key_runs_and_the_batched_histogram_compose_on_the_device(G):
    """Sort by key -> key runs -> the batched histogram of the values on the offsets key runs wrote, nothing read on the host in
    between, against numpy's group-by."""
    import torch

    rng = np.random.default_rng(44)
    n, alphabet, max_runs, bins = 200000, 300, 512, 64
    keys = (rng.zipf(1.2, n) % alphabet).astype(np.uint32) * np.uint32(7919)  # groups of very different sizes
    vals = rng.integers(0, 64 * 5, n, dtype=np.uint32)
    kt, vt = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    ft = torch.zeros(max_runs + 1, dtype=torch.int32, device="cuda")
    nt = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((max_runs * bins,), -1, dtype=torch.int32, device="cuda")
    h = G.Histogram()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "uint32")
    G.KeyRuns().run_ptr(kt.data_ptr(), n, ft.data_ptr(), max_runs, nt.data_ptr())
    h.run_batch_offsets_even_ptr(vt.data_ptr(), n, ft.data_ptr(), max_runs, 0, 64 * 5, bins, out.data_ptr(), "uint32", False, None)
    G.synchronize()
    torch.cuda.synchronize()
    present = np.unique(keys)
    got = out.cpu().numpy().view(np.uint32).reshape(max_runs, bins)
    assert int(nt.cpu()[0]) == present.size
    for r, k in enumerate(present):
        assert (got[r] == np.bincount(vals[keys == k] // 5, minlength=bins)).all(), r
    assert (got[present.size:] == 0).all()  # key runs pads the offsets with n: the segments behind the last run are empty


def test_the_cpp_surface(G):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_histogram_batch_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
