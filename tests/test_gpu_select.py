"""GPU tests of select (glu_select_run_ptr): stable stream compaction by a stencil and a comparison -- the indices of the selected
elements, the items at them and their number.  Expected values come from numpy: idx = flatnonzero(op(stencil, threshold)) and
items[idx]; every comparison is `==`, select is exact.  Every array the call writes sits inside an allocation with poison in front
of it and behind it, and is itself filled with poison first, so that an entry the call must not touch still holds it.  Sizes come
from plan_select."""
import ctypes
import gc
import operator
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes of poison in front of and behind an array, inside its allocation
POISON = 0xA5

STENCILS = {"float": (0, np.float32), "double": (1, np.float64), "int": (2, np.int32), "uint": (3, np.uint32), "byte": (12, np.uint8)}
OPS = [operator.eq, operator.ne, operator.lt, operator.le, operator.gt, operator.ge]  # GLU_SELECT_EQ .. GLU_SELECT_GE
EQ, NE, LT, LE, GT, GE = range(6)


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


def selected(stencil, op, threshold):
    """numpy's answer; the threshold in the stencil's type (None: zero)."""
    t = stencil.dtype.type(0 if threshold is None else threshold)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(OPS[op](stencil, t))


def check_case(G, sel, stencil, op=NE, threshold=None, max_out=None, items=None, item_bytes=4, with_indices=True, with_items=True,
               stencil_shift=0, items_shift=0, items_are_stencil=False):
    """One call on `stencil` (numpy, one of the five types); `items`: uint8 of count * item_bytes bytes (made here if None).  Every
    output compared with `==`, the poison checked, the inputs unchanged.  Returns the number selected."""
    import torch

    n = stencil.size
    stencil_type = next(v[0] for v in STENCILS.values() if v[1] == stencil.dtype.type)
    max_out = n if max_out is None else max_out
    sa = Array(stencil, stencil_shift)
    if items_are_stencil:
        item_bytes, items, ia = stencil.dtype.itemsize, stencil.view(np.uint8), sa
    elif with_items:
        if items is None:
            items = np.random.default_rng(n + item_bytes).integers(0, 256, n * item_bytes, dtype=np.uint8)
        ia = Array(items, items_shift)
    oi = Array.poisoned(max_out * item_bytes) if with_items else Array.poisoned(64)
    ox = Array.poisoned(max_out * 4)
    na = Array.poisoned(4)
    sel.run_ptr(sa.ptr if n else None, n, max_out, na.ptr, out_indices_ptr=ox.ptr if with_indices else None,
                items_ptr=ia.ptr if with_items else None, out_items_ptr=oi.ptr if with_items else None, item_bytes=item_bytes,
                stencil_type=stencil_type, op=op, threshold=threshold, stream=stream())
    torch.cuda.synchronize()
    idx = selected(stencil, op, threshold)
    m = min(idx.size, max_out)
    what = (str(stencil.dtype), n, op, threshold, max_out, item_bytes, stencil_shift, items_shift)
    assert int(na.result(np.uint32)[0]) == idx.size, what
    want = np.full(max_out, 0xA5A5A5A5, dtype=np.uint32)
    if with_indices:
        want[:m] = idx[:m]
    got = ox.result(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    got = oi.result(np.uint8)
    want = np.full(got.size, POISON, dtype=np.uint8)
    if with_items:
        want[:m * item_bytes] = items.reshape(n, item_bytes)[idx[:m]].ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]) // item_bytes, int(got[bad[0]]), int(want[bad[0]]))
    assert (sa.result(np.uint8) == stencil.view(np.uint8)).all(), "the call wrote to its stencil"
    if with_items and not items_are_stencil:
        assert (ia.result(np.uint8) == items).all(), "the call wrote to its items"
    return idx.size


PATTERNS = ["none", "all", "half", "one_in_1000", "tile_firsts", "tile_lasts", "lane0", "first", "last"]


def flags_of(name, rng, n, tile, wave_elems):
    i = np.arange(n)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "half":
        return rng.integers(0, 2, n).astype(bool)
    if name == "one_in_1000":
        return rng.integers(0, 1000, n) == 0
    if name == "tile_firsts":
        return i % tile == 0
    if name == "tile_lasts":
        return i % tile == tile - 1
    if name == "lane0":  # lane 0 of a wave holds the first element of each of its packs: the multiples of a sixteenth of the wave's part
        return i % wave_elems == 0
    if name == "first":
        return i == 0
    return i == n - 1


def as_stencil(flags, dtype, rng):
    """A stencil of `dtype` that is nonzero exactly where `flags` is set (nonzero values of both signs and of every byte)."""
    if dtype == np.uint8:
        v = rng.integers(1, 256, flags.size).astype(np.uint8)
    elif dtype in (np.float32, np.float64):
        v = (rng.integers(1, 1000, flags.size) * rng.choice([-1, 1], flags.size)).astype(dtype) / dtype(8)
    elif dtype == np.int32:
        v = (rng.integers(1, 2**31, flags.size) * rng.choice([-1, 1], flags.size)).astype(np.int32)
    else:
        v = rng.integers(1, 2**32, flags.size, dtype=np.uint32)
    return np.where(flags, v, dtype(0)).astype(dtype)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("stencil", sorted(STENCILS))
def test_boundaries(G, stencil, name):
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select(1, stencil_type)[0]
    wave_elems = 64 * (16 // np.dtype(dtype).itemsize)  # the elements one load instruction of a wave covers
    rng = np.random.default_rng(PATTERNS.index(name) + 100 * stencil_type)
    sel = G.Select()
    for n in (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1):
        flags = flags_of(name, rng, n, tile, wave_elems)
        got = check_case(G, sel, as_stencil(flags, dtype, rng))
        assert got == int(flags.sum())
        if name == "all":
            assert got == n
        if name in ("first", "last"):
            assert got == min(n, 1)


@pytest.mark.parametrize("item_bytes", [4, 8, 16, 32])
def test_item_sizes(G, item_bytes):
    tile = G.plan_select(1, 3)[0]
    rng = np.random.default_rng(item_bytes)
    sel = G.Select()
    for n in (tile + 77, 2 * tile + 1):
        for name in ("half", "all"):
            stencil = as_stencil(flags_of(name, rng, n, tile, 256), np.uint32, rng)
            assert check_case(G, sel, stencil, item_bytes=item_bytes) > n // 3
        mask = as_stencil(flags_of("half", rng, n, tile, 1024), np.uint8, rng)
        check_case(G, sel, mask, item_bytes=item_bytes)


def test_items_may_be_the_stencil_and_either_output_may_be_skipped(G):
    rng = np.random.default_rng(11)
    sel = G.Select()
    for dtype, threshold in ((np.float32, 0.25), (np.float64, -0.5), (np.int32, -7), (np.uint32, 1 << 31), (np.uint8, 100)):
        tile = G.plan_select(1, next(v[0] for v in STENCILS.values() if v[1] == dtype))[0]
        n = tile + 77
        stencil = as_stencil(flags_of("all", rng, n, tile, 1), dtype, rng)
        if dtype != np.uint8:  # (an item is 4, 8, 16 or 32 bytes: a byte stencil cannot be its own items)
            assert 0 < check_case(G, sel, stencil, op=GT, threshold=threshold, items_are_stencil=True) < n
        assert 0 < check_case(G, sel, stencil, op=LE, threshold=threshold, with_indices=False, item_bytes=8) < n  # only items
        assert 0 < check_case(G, sel, stencil, op=GE, threshold=threshold, with_items=False) < n  # only indices
        assert 0 < check_case(G, sel, stencil, op=LT, threshold=threshold, with_items=False, with_indices=False) < n  # only the count


def alphabet_of(dtype, threshold):
    if dtype in (np.float32, np.float64):
        nan2 = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0] if dtype == np.float32 else \
            np.array([0xFFF8000000012345], dtype=np.uint64).view(np.float64)[0]
        t = dtype(threshold)
        return np.array([-np.inf, -2.25, -0.0, 0.0, np.finfo(dtype).smallest_subnormal, t, np.nextafter(t, dtype(-np.inf)),
                         np.nextafter(t, dtype(np.inf)), np.inf, np.nan, nan2], dtype=dtype)
    if dtype == np.uint8:
        return np.array([0, 1, 127, 128, 255], dtype=np.uint8)
    bits = np.array([0x80000000, 0xFFFFFFFF, 0, 1, 0x7FFFFFFF], dtype=np.uint32)  # INT_MIN, -1, 0, 1, INT_MAX
    near = np.array([threshold - 1, threshold, threshold + 1], dtype=np.int64).astype(dtype)
    return np.concatenate([bits.view(dtype), near])


@pytest.mark.parametrize("stencil", sorted(STENCILS))
def test_comparisons(G, stencil):
    """All six comparisons on stencils drawn from a small alphabet that holds the threshold, its neighbours and the type's
    extremes; IEEE semantics for floats (a NaN passes only NE; -0.0 == +0.0), signed for int, unsigned for uint and byte; a NULL
    threshold is a zero threshold."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select(1, stencil_type)[0]
    n = tile + 77
    rng = np.random.default_rng(200 + stencil_type)
    sel = G.Select()
    if dtype in (np.float32, np.float64):
        thresholds = [1.5, 0.0, float("nan")]
    elif dtype == np.uint8:
        thresholds = [0, 1, 127, 128, 255]
    elif dtype == np.int32:
        thresholds = [-1000, 0, -(1 << 31), (1 << 31) - 1]
    else:
        thresholds = [1000, 0, 1, 0x80000000, 0xFFFFFFFF]
    for threshold in thresholds:
        alphabet = alphabet_of(dtype, 1.5 if threshold != threshold else threshold)
        data = alphabet[rng.integers(0, alphabet.size, n)]
        data[:alphabet.size] = alphabet  # (every letter is there)
        counts = [check_case(G, sel, data, op=op, threshold=threshold, item_bytes=16) for op in range(6)]
        assert counts[EQ] + counts[NE] == n
        if threshold != threshold:  # NaN: only NE selects anything
            assert counts == [0, n, 0, 0, 0, 0]
        elif dtype in (np.float32, np.float64):
            nans = int(np.isnan(data).sum())
            assert nans > 0 and counts[LT] + counts[GE] == n - nans and counts[LE] + counts[GT] == n - nans
            if threshold == 0.0:
                neg_zero = np.flatnonzero(np.signbit(data) & (data == 0))
                assert neg_zero.size > 0 and counts[EQ] == int((data == 0).sum()) >= neg_zero.size + 1  # -0.0 EQ +0.0 selects
        else:
            assert counts[LT] + counts[GE] == n and counts[LE] + counts[GT] == n
        if threshold == 0:
            for op in range(6):
                assert check_case(G, sel, data, op=op, threshold=None, with_items=False) == counts[op]
            if dtype == np.int32:
                assert counts[LT] == int((data.view(np.uint32) >= 0x80000000).sum()) > 0  # LT 0 selects the negatives: a signed compare
        if dtype == np.uint32 and threshold == 1:
            assert counts[GT] >= int((data == 0x80000000).sum()) > 0 and counts[GT] == int((data > 1).sum())  # 0x80000000 GT 1: unsigned


@pytest.mark.parametrize("stencil", ["uint", "byte", "double"])
def test_capacity(G, stencil):
    """max_out below, at and above the number selected: *num_selected is the true number every time and the entries at or behind
    min(S, max_out) are still poison (check_case expects it there)."""
    stencil_type, dtype = STENCILS[stencil]
    rng = np.random.default_rng(20)
    data = as_stencil(rng.integers(0, 3, 3000) == 0, dtype, rng)
    S = int((data != 0).sum())
    assert 800 < S < 1300
    sel = G.Select()
    for max_out in (0, 1, S - 1, S, S + 1, S + 4097):
        assert check_case(G, sel, data, max_out=max_out, item_bytes=8) == S


@pytest.mark.parametrize("stencil,shift", [("float", 1), ("int", 2), ("uint", 3), ("double", 1), ("byte", 1), ("byte", 7), ("byte", 15)])
def test_misaligned_bases(G, stencil, shift):
    """A stencil that starts `shift` elements behind a 16-byte boundary: the tiles are counted from that boundary, so the last
    tile's elements move too (2 * tile elements: a tile more than the plan's when the base is not aligned).  The items are
    shifted on their own, by one item."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select(1, stencil_type)[0]
    size = np.dtype(dtype).itemsize
    rng = np.random.default_rng(30 + shift)
    sel = G.Select()
    assert Array(np.zeros(1, dtype=dtype), shift * size).ptr % 16 == shift * size
    for n in (tile + 5, 2 * tile - 1, 2 * tile):
        if n == 2 * tile:
            assert G.plan_select(n, stencil_type)[1] == 2 and -(-(n + shift) // tile) == 3
        for name in ("half", "all", "tile_firsts", "tile_lasts"):
            data = as_stencil(flags_of(name, rng, n, tile, 1), dtype, rng)
            for item_bytes, items_shift in ((4, 4), (8, 8), (16, 0)):
                assert Array(np.zeros(item_bytes, dtype=np.uint8), items_shift).ptr % 16 == items_shift
                check_case(G, sel, data, item_bytes=item_bytes, stencil_shift=shift * size, items_shift=items_shift)


@pytest.mark.parametrize("more_tiles", [0, 1])
def test_two_rounds_of_the_count_scan(G, more_tiles):
    """The smallest count whose tile counts take two rounds of their scan (and, second case, a tile and three elements more, so
    that the second round's first tile is full), a byte stencil.  One in 1000 selected, plus the first and the last element of the
    second round's first tile; indices only."""
    import torch

    B = G.SelectStencil_Byte
    tile = G.plan_select(1, B)[0]
    lo, hi = 1, 1 << 31  # rounds(lo) < 2 <= rounds(hi)
    assert G.plan_select(hi, B)[2] >= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if G.plan_select(mid, B)[2] >= 2:
            hi = mid
        else:
            lo = mid
    assert G.plan_select(hi, B)[2] == 2 and G.plan_select(hi - 1, B)[2] == 1
    first = G.plan_select(hi - 1, B)[1] * tile  # the first element of the second round's first tile
    n = hi + more_tiles * (tile + 3)
    assert first < n < 1 << 26 and G.plan_select(n, B)[2] == 2
    mask = np.zeros(n, dtype=np.uint8)
    mask[::1000] = 1
    mask[first] = 255
    mask[min(first + tile, n) - 1] = 128
    idx = np.flatnonzero(mask)
    max_out = idx.size + 7
    mt = torch.from_numpy(mask).cuda()
    ox, na = Array.poisoned(max_out * 4), Array.poisoned(4)
    G.Select().run_ptr(mt.data_ptr(), n, max_out, na.ptr, out_indices_ptr=ox.ptr, stencil_type=B, stream=stream())
    torch.cuda.synchronize()
    assert int(na.result(np.uint32)[0]) == idx.size
    want = np.full(max_out, 0xA5A5A5A5, dtype=np.uint32)
    want[:idx.size] = idx
    got = ox.result(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert (mt.cpu().numpy() == mask).all()
    del mt
    torch.cuda.empty_cache()


def test_argument_checks_and_overlaps(G):
    """One call per case the host can check, each with its own message; a witness buffer (every output lies in it) shows that the
    refused calls wrote nothing.  Outputs that only touch the inputs are accepted and correct; no elements: only *num_selected."""
    import torch

    sel = G.Select()
    n = 4096
    rng = np.random.default_rng(60)
    data = rng.integers(0, 2**32, n, dtype=np.uint32)
    st = torch.from_numpy(data.view(np.int32).copy()).cuda()          # the stencil
    it = torch.from_numpy(data.view(np.int32).copy()).cuda()          # the items
    wt = torch.zeros(4 * n, dtype=torch.int32, device="cuda")        # the witness: out_items, out_indices, num_selected
    sp, ip, wp = st.data_ptr(), it.data_ptr(), wt.data_ptr()
    oi, ox, nu = wp, wp + 4 * n, wp + 8 * n
    L, vp = G.lib(), ctypes.c_void_p
    U = G.SelectStencil_Uint

    def run(stencil=sp, count=64, max_out=64, num=nu, indices=ox, items=ip, out_items=oi, item_bytes=4, stencil_type=U, op=NE):
        sel.run_ptr(stencil, count, max_out, num, indices, items, out_items, item_bytes, stencil_type, op)

    bad = [
        (lambda: G.check(L.glu_select_run_ptr(None, vp(sp), U, NE, None, 64, vp(ip), 4, vp(oi), vp(ox), 64, vp(nu), None)), "select is NULL"),
        (lambda: G.check(L.glu_select_prepare(None, 64, U)), "select is NULL"),
        (lambda: G.check(L.glu_select_create(None)), "out is NULL"),
        (lambda: run(stencil=None), "Invalid stencil buffer"),
        (lambda: run(num=None), "Invalid num_selected pointer"),
        (lambda: run(items=None), "items and out_items must both"),
        (lambda: run(out_items=None), "items and out_items must both"),
        (lambda: run(stencil_type=G.DataType_Vec4), "stencil_type"),
        (lambda: run(stencil_type=13), "stencil_type"),
        (lambda: run(stencil_type=-1), "stencil_type"),
        (lambda: run(op=6), "op must be"),
        (lambda: run(op=-1), "op must be"),
        (lambda: run(item_bytes=12), "item_bytes must be"),
        (lambda: run(item_bytes=0), "item_bytes must be"),
        (lambda: run(item_bytes=64), "item_bytes must be"),
        (lambda: run(stencil=sp + 2), "stencil is not aligned"),
        (lambda: run(stencil=sp + 4, stencil_type=G.SelectStencil_Double), "stencil is not aligned"),
        (lambda: run(items=ip + 4, item_bytes=8), "items is not aligned"),
        (lambda: run(items=ip + 8, item_bytes=32), "items is not aligned"),
        (lambda: run(out_items=oi + 8, item_bytes=16), "out_items is not aligned"),
        (lambda: run(indices=ox + 2), "out_indices is not aligned"),
        (lambda: run(num=nu + 1), "num_selected is not aligned"),
        (lambda: run(count=1 << 32), "count below 2^32"),
        (lambda: run(max_out=1 << 32), "max_out must be below 2^32"),
        (lambda: sel.prepare(1 << 32), "count below 2^32"),
        (lambda: sel.prepare(64, 5), "stencil_type"),
        (lambda: G.plan_select(8, 4), "stencil_type"),
        (lambda: run(out_items=sp + 128), "out_items overlaps stencil"),
        (lambda: run(out_items=ip + 252), "out_items overlaps items"),
        (lambda: run(indices=sp - 4 * 63), "out_indices overlaps stencil"),
        (lambda: run(indices=ip), "out_indices overlaps items"),
        (lambda: run(num=sp + 252), "num_selected overlaps stencil"),
        (lambda: run(num=ip), "num_selected overlaps items"),
        (lambda: run(items=sp, out_items=sp + 16), "out_items overlaps stencil"),
    ]
    assert len({m for _, m in bad}) == 21  # (the messages are distinct)
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (st.cpu().numpy().view(np.uint32) == data).all() and (it.cpu().numpy().view(np.uint32) == data).all()
    # no elements: NULL stencil is fine, *num_selected = 0 and nothing else written
    wt.fill_(-1)
    sel.run_ptr(None, 0, 64, nu, ox, ip, oi, 4, U, NE, stream=stream())
    torch.cuda.synchronize()
    got = wt.cpu().numpy()
    assert got[2 * n] == 0
    got[2 * n] = -1
    assert (got == -1).all()
    # arrays that only touch the inputs are fine: the stencil is the middle of a buffer, the indices end where it begins, the items
    # written begin where it ends (and a max_out far above the count does not make them overlap: min(count, max_out) entries count)
    part = data[100:n - 100]
    idx = np.flatnonzero(part > np.uint32(0xE0000000))
    assert 99 < idx.size < n - 200
    sel.run_ptr(sp + 400, n - 200, 100, nu, sp, ip + 400, sp + 4 * (n - 100), 4, U, GT, 0xE0000000, stream())
    torch.cuda.synchronize()
    got = st.cpu().numpy().view(np.uint32)
    assert int(wt.cpu().numpy().view(np.uint32)[2 * n]) == idx.size
    assert (got[100:n - 100] == part).all()
    assert (got[:100] == idx[:100]).all()
    assert (got[n - 100:] == part[idx[:100]]).all()
    sel.run_ptr(sp + 400, 50, 1 << 31, nu, ox, ip, sp + 400 + 200, 4, U, GE, 0, stream())  # (50 items written at most, behind the 50 read)
    torch.cuda.synchronize()
    assert (st.cpu().numpy().view(np.uint32)[150:200] == data[:50]).all()


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed on
    three stencil contents with about 50 %, 10 % and 0.1 % selected (the first two above max_out): the launch sequence does not
    depend on the data."""
    import torch

    F = G.SelectStencil_Float
    tile = G.plan_select(1, F)[0]
    n = 37 * tile + 11
    max_out = n // 20  # between the 10 % of the second and the 0.1 % of the third contents
    rng = np.random.default_rng(90)
    sel = G.Select()
    st = torch.empty(n, dtype=torch.float32, device="cuda")
    it = torch.from_numpy(rng.integers(0, 2**31, 2 * n).astype(np.int32)).cuda()  # 8-byte items
    items = it.cpu().numpy().view(np.uint64)
    oi = torch.empty(2 * max_out, dtype=torch.int32, device="cuda")
    ox = torch.empty(max_out, dtype=torch.int32, device="cuda")
    nt = torch.empty(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(data):
        st.copy_(torch.from_numpy(data))
        oi.fill_(-1515870811)
        ox.fill_(-1515870811)
        nt.fill_(-1515870811)

    def verify(data):
        idx = np.flatnonzero(data > np.float32(0.5))
        m = min(idx.size, max_out)
        assert int(nt.cpu().numpy().view(np.uint32)[0]) == idx.size
        want = np.full(max_out, 0xA5A5A5A5, dtype=np.uint32)
        want[:m] = idx[:m]
        assert (ox.cpu().numpy().view(np.uint32) == want).all()
        want = np.full(max_out, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        want[:m] = items[idx[:m]]
        assert (oi.cpu().numpy().view(np.uint64) == want).all()
        return idx.size

    def call(s):
        sel.run_ptr(st.data_ptr(), n, max_out, nt.data_ptr(), ox.data_ptr(), it.data_ptr(), oi.data_ptr(), 8, F, GT, 0.5, s)

    def contents(share):  # uniform in [0, 1): above 0.5 with probability `share`
        return (rng.random(n, dtype=np.float32) * np.float32(0.5 / (1.0 - share))).astype(np.float32) if share < 0.5 else \
            rng.random(n, dtype=np.float32)

    with torch.cuda.stream(side):
        data = contents(0.5)
        fill(data)
        side.synchronize()
        sel.prepare(n, F)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(data)
        fill(data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        seen = []
        for share in (0.5, 0.1, 0.001):
            data = contents(share)
            fill(data)
            graph.replay()
            side.synchronize()
            seen.append(verify(data))
        assert seen[0] > seen[1] > max_out > seen[2] > 0, (seen, max_out)
        assert 0.45 * n < seen[0] < 0.55 * n and 0.08 * n < seen[1] < 0.12 * n and seen[2] < 0.002 * n


def test_with_the_family(G):
    """Sort (key, value) pairs, key runs, a batched reduce (Sum) of the values per run, then select the unique keys and the sums
    whose sum is above a threshold -- four calls on one stream with no host read in between, against a numpy group-by."""
    import torch

    rng = np.random.default_rng(70)
    n, distinct, max_runs = 20011, 300, 320
    keys = (rng.integers(0, distinct, n).astype(np.uint32) * np.uint32(7919))
    vals = rng.integers(0, 1000, n, dtype=np.uint32)
    kt = torch.from_numpy(keys.view(np.int32)).cuda()
    vt = torch.from_numpy(vals.view(np.int32)).cuda()
    offsets, unique, sums, runs_n = (Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4 * max_runs), Array.poisoned(4 * max_runs),
                                     Array.poisoned(4))
    kept_keys, kept_sums, kept_n, kept_n2 = Array.poisoned(4 * max_runs), Array.poisoned(4 * max_runs), Array.poisoned(4), Array.poisoned(4)
    present = np.unique(keys)
    group_sums = np.array([int(vals[keys == k].sum()) for k in present], dtype=np.uint32)
    threshold = int(np.median(group_sums))
    s = stream()
    sel = G.Select()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "uint32", s)
    G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum).run_by_key_ptr(G.KeyRuns(), kt.data_ptr(), vt.data_ptr(), sums.ptr, n, offsets.ptr,
                                                                  max_runs, runs_n.ptr, unique.ptr, stream=s)
    # (the entries of sums behind the last run are the sums of empty segments, 0: below the threshold)
    sel.run_ptr(sums.ptr, max_runs, max_runs, kept_n.ptr, items_ptr=unique.ptr, out_items_ptr=kept_keys.ptr, op=GT, threshold=threshold, stream=s)
    sel.run_ptr(sums.ptr, max_runs, max_runs, kept_n2.ptr, items_ptr=sums.ptr, out_items_ptr=kept_sums.ptr, op=GT, threshold=threshold, stream=s)
    torch.cuda.synchronize()
    assert int(runs_n.result(np.uint32)[0]) == present.size
    keep = group_sums > threshold
    assert present.size // 3 < int(keep.sum()) < 2 * present.size // 3 + 1
    assert int(kept_n.result(np.uint32)[0]) == int(keep.sum()) == int(kept_n2.result(np.uint32)[0])
    m = int(keep.sum())
    got_keys, got_sums = kept_keys.result(np.uint32), kept_sums.result(np.uint32)
    assert (got_keys[:m] == present[keep]).all() and (got_keys[m:] == 0xA5A5A5A5).all()
    assert (got_sums[:m] == group_sums[keep]).all() and (got_sums[m:] == 0xA5A5A5A5).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_select_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
