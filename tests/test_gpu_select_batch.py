"""GPU tests of the batched select (glu_select_run_batch_ptr, glu_select_run_batch_offsets_ptr): the single select's compaction
over the elements between the first and the last boundary of a list of segments, the offsets of the compacted segments, and indices
local to the segment.  Expected values are a numpy restatement of the contract in glu_hip.h (`expected`), malformed offsets included;
every comparison is `==`, select is exact.  Every array the call writes sits inside an allocation with poison in front of it and
behind it, and is itself filled with poison first, so that an entry the call must not touch still holds it.  Sizes come from
plan_select_batch."""
import gc
import hashlib
import operator
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes of poison in front of and behind an array, inside its allocation
POISON = 0xA5
POISON32 = 0xA5A5A5A5

STENCILS = {"float": (0, np.float32), "double": (1, np.float64), "int": (2, np.int32), "uint": (3, np.uint32), "byte": (12, np.uint8)}
OPS = [operator.eq, operator.ne, operator.lt, operator.le, operator.gt, operator.ge]  # GLU_SELECT_EQ .. GLU_SELECT_GE
EQ, NE, LT, LE, GT, GE = range(6)
GLOBAL, LOCAL = 0, 1
PATTERNS = ["none", "all", "half", "one_in_1000", "tile_firsts", "tile_lasts", "lane0", "first", "last"]


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


def expected(flags, bounds, max_out):
    """The contract: (the indices of the selected elements, their segment-local indices, out_offsets, S).  `flags`: stencil OP
    threshold per element; `bounds`: the offsets as given (or s * count).  The local indices mean something for sorted offsets only."""
    total = flags.size
    b = np.minimum(np.asarray(bounds, dtype=np.int64), total)
    i = np.arange(total)
    chosen = flags & (i >= b[0]) & (i < b[-1])
    idx = np.flatnonzero(chosen)
    rank = np.concatenate([[0], np.cumsum(chosen)])
    seg = np.searchsorted(b, idx, "right") - 1
    return idx, idx - b[seg], np.minimum(max_out, rank[b]).astype(np.uint32), idx.size


def flags_from(stencil, op, threshold):
    t = stencil.dtype.type(0 if threshold is None else threshold)
    with np.errstate(invalid="ignore"):
        return OPS[op](stencil, t)


def check_case(G, sel, stencil, offsets=None, partition=None, op=NE, threshold=None, max_out=None, form=GLOBAL, item_bytes=4,
               with_indices=True, with_items=True, with_offsets=True, stencil_shift=0, items_shift=0, items_are_stencil=False, sorted_offsets=True):
    """One call on `stencil` (numpy, one of the five types) over `offsets` (numpy uint32) or equal partitions of `partition`.  Every
    output compared with `==`, the poison checked, the inputs unchanged.  Returns (S, out_offsets)."""
    import torch

    n = stencil.size
    stencil_type = next(v[0] for v in STENCILS.values() if v[1] == stencil.dtype.type)
    if offsets is None:
        parts = n // partition if partition else 0
        assert parts * (partition or 0) == n
        bounds = np.arange(parts + 1, dtype=np.int64) * (partition or 0)
    else:
        parts, bounds = offsets.size - 1, offsets
    idx, local, want_offsets, S = expected(flags_from(stencil, op, threshold), bounds, n if max_out is None else max_out)
    max_out = n if max_out is None else max_out
    sa = Array(stencil, stencil_shift)
    if items_are_stencil:
        item_bytes, items, ia = stencil.dtype.itemsize, stencil.view(np.uint8), sa
    elif with_items:
        items = np.random.default_rng(n + item_bytes).integers(0, 256, n * item_bytes, dtype=np.uint8)
        ia = Array(items, items_shift)
    oi = Array.poisoned(max_out * item_bytes) if with_items else Array.poisoned(64)
    ox, oo, na = Array.poisoned(max_out * 4), Array.poisoned((parts + 1) * 4), Array.poisoned(4)
    common = dict(out_indices_ptr=ox.ptr if with_indices else None, items_ptr=ia.ptr if with_items else None,
                  out_items_ptr=oi.ptr if with_items else None, item_bytes=item_bytes, out_offsets_ptr=oo.ptr if with_offsets else None,
                  index_form=form, stencil_type=stencil_type, op=op, threshold=threshold, stream=stream())
    if offsets is None:
        sel.run_batch_ptr(sa.ptr if n else None, partition or 0, parts, max_out, na.ptr, **common)
    else:
        fa = Array(offsets)
        sel.run_batch_offsets_ptr(sa.ptr if n else None, n, fa.ptr, parts, max_out, na.ptr, **common)
    torch.cuda.synchronize()
    m = min(S, max_out)
    what = (str(stencil.dtype), n, parts, op, threshold, max_out, form, item_bytes, stencil_shift, items_shift)
    assert int(na.result(np.uint32)[0]) == S, what
    got = oo.result(np.uint32)
    want = want_offsets if with_offsets and parts else np.full(parts + 1, POISON32, dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "out_offsets", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    got = ox.result(np.uint32)
    want = np.full(max_out, POISON32, dtype=np.uint32)
    if with_indices:
        want[:m] = (local if form == LOCAL else idx)[:m]
    if form == LOCAL and not sorted_offsets:  # (unspecified values, in the entries that are written and nowhere else)
        got[:m] = want[:m]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "out_indices", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    got = oi.result(np.uint8)
    want = np.full(got.size, POISON, dtype=np.uint8)
    if with_items:
        want[:m * item_bytes] = items.reshape(n, item_bytes)[idx[:m]].ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "out_items", int(bad[0]) // item_bytes, int(got[bad[0]]), int(want[bad[0]]))
    assert (sa.result(np.uint8) == stencil.view(np.uint8)).all(), "the call wrote to its stencil"
    if with_items and not items_are_stencil:
        assert (ia.result(np.uint8) == items).all(), "the call wrote to its items"
    if offsets is not None:
        assert (fa.result(np.uint32) == offsets).all(), "the call wrote to its offsets"
    return S, want_offsets


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
    if name == "lane0":
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


def u32(values):
    return np.asarray(values, dtype=np.uint32)


def layouts(total, tile, empties=False):
    """{name: sorted offsets} over `total` elements: the segment shapes that can go wrong."""
    out = {"one": u32([0, total]), "per_element": np.arange(total + 1, dtype=np.uint32)}
    edges = sorted({0, total} | {p for k in range(total // tile + 2) for p in (k * tile - 1, k * tile, k * tile + 1) if 0 <= p <= total})
    out["tile_edges"] = u32(edges)
    out["wave_parts"] = u32(sorted(set(range(0, total, tile // 4)) | {total}))
    if total > 14:
        out["partial"] = u32([5, 5, total // 2, total - 9])  # offsets[0] > 0 and offsets[n] < total: the elements outside keep poison
        out["padded"] = u32([0, 3, total // 3, total] + [total] * 9)  # key runs' own: the tail filled with the count
    if empties and total > tile // 2 + 3:
        out["empties_inside"] = u32([0] + [tile // 2 + 3] * (1 << 16) + [total])
    if empties and total >= tile:
        out["empties_on_edge"] = u32([0] + [tile] * (1 << 16) + [total])
    return out


@pytest.mark.parametrize("stencil", sorted(STENCILS))
def test_totals_and_segment_shapes(G, stencil):
    """Every total where the tiles change, under every segment shape, half of the elements selected; all three outputs in both
    forms (8-byte items)."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    assert tile == {4: 4096, 8: 2048, 1: 4096}[np.dtype(dtype).itemsize]
    rng = np.random.default_rng(stencil_type)
    sel = G.Select()
    for total in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 17):
        data = as_stencil(flags_of("half", rng, total, tile, 1), dtype, rng)
        for name, offsets in layouts(total, tile, empties=total in (tile, 3 * tile + 17)).items():
            for form in (GLOBAL, LOCAL):
                S, out = check_case(G, sel, data, offsets, form=form, item_bytes=8)
                assert out.size == offsets.size and out[-1] == S
                assert S == int((data[5:total - 9] != 0).sum()) if name == "partial" else S == int((data != 0).sum())
                if name.startswith("empties"):
                    assert (out[1:-1] == out[1]).all() and 0 < out[1] <= S  # an emptied segment stays an empty segment


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("stencil", sorted(STENCILS))
def test_flag_patterns(G, stencil, name):
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    wave_elems = 64 * (16 // np.dtype(dtype).itemsize)
    rng = np.random.default_rng(PATTERNS.index(name) + 100 * stencil_type)
    sel = G.Select()
    for total in (tile - 1, tile + 1, 3 * tile + 17):
        flags = flags_of(name, rng, total, tile, wave_elems)
        data = as_stencil(flags, dtype, rng)
        for lay in ("tile_edges", "wave_parts", "partial"):
            S, _ = check_case(G, sel, data, layouts(total, tile)[lay], form=LOCAL)
            if lay != "partial":
                assert S == int(flags.sum())


@pytest.mark.parametrize("count", ["1", "255", "T", "T+1"])
@pytest.mark.parametrize("stencil", ["uint", "double", "byte"])
def test_equal_partitions(G, stencil, count):
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    count, parts = {"1": (1, tile + 3), "255": (255, 37), "T": (tile, 3), "T+1": (tile + 1, 3)}[count]
    rng = np.random.default_rng(count)
    data = as_stencil(flags_of("half", rng, count * parts, tile, 1), dtype, rng)
    sel = G.Select()
    for form in (GLOBAL, LOCAL):
        S, out = check_case(G, sel, data, partition=count, form=form)
        assert out[0] == 0 and out[-1] == S
    check_case(G, sel, data, partition=count, form=LOCAL, max_out=S // 2, with_items=False)
    check_case(G, sel, data[:0], partition=count)  # no partitions: *num_selected = 0 and nothing else
    check_case(G, sel, data[:0], partition=0)


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
    """All six comparisons on stencils drawn from a small alphabet that holds the threshold, its neighbours and the type's extremes
    (NaN and both zeros among the floats), over a partial cover; a NULL threshold is a zero threshold."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    n = tile + 77
    rng = np.random.default_rng(200 + stencil_type)
    sel = G.Select()
    offsets = u32([3, 40, 40, tile - 1, tile + 5, n - 2])
    thresholds = [1.5, 0.0, float("nan")] if dtype in (np.float32, np.float64) else [0, 1, 128, 255] if dtype == np.uint8 else \
        [-1000, 0, -(1 << 31), (1 << 31) - 1] if dtype == np.int32 else [1000, 0, 0x80000000, 0xFFFFFFFF]
    for threshold in thresholds:
        alphabet = alphabet_of(dtype, 1.5 if threshold != threshold else threshold)
        data = alphabet[rng.integers(0, alphabet.size, n)]
        data[3:3 + alphabet.size] = alphabet  # (every letter is there, inside the cover)
        counts = [check_case(G, sel, data, offsets, op=op, threshold=threshold, item_bytes=16, form=LOCAL)[0] for op in range(6)]
        assert counts[EQ] + counts[NE] == n - 5
        if threshold != threshold:  # NaN: only NE selects anything
            assert counts == [0, n - 5, 0, 0, 0, 0]
        if threshold == 0:
            for op in range(6):
                assert check_case(G, sel, data, offsets, op=op, threshold=None, with_items=False)[0] == counts[op]


@pytest.mark.parametrize("item_bytes", [4, 8, 16, 32])
def test_item_widths_and_every_subset_of_the_outputs(G, item_bytes):
    tile = G.plan_select_batch(1, 1, 3)[0]
    rng = np.random.default_rng(item_bytes)
    sel = G.Select()
    n = 2 * tile + 77
    data = as_stencil(flags_of("half", rng, n, tile, 1), np.uint32, rng)
    mask = as_stencil(flags_of("half", rng, n, tile, 1), np.uint8, rng)
    offsets = layouts(n, tile)["tile_edges"]
    for form in (GLOBAL, LOCAL):
        for with_indices in (False, True):
            for with_items in (False, True):
                for with_offsets in (False, True):
                    for stencil in (data, mask):
                        check_case(G, sel, stencil, offsets, form=form, item_bytes=item_bytes, with_indices=with_indices, with_items=with_items,
                                   with_offsets=with_offsets)


def test_items_may_be_the_stencil(G):
    rng = np.random.default_rng(11)
    sel = G.Select()
    for dtype, threshold in ((np.float32, 0.25), (np.float64, -0.5), (np.int32, -7), (np.uint32, 1 << 31)):
        tile = G.plan_select_batch(1, 1, next(v[0] for v in STENCILS.values() if v[1] == dtype))[0]
        n = tile + 77
        data = as_stencil(flags_of("all", rng, n, tile, 1), dtype, rng)
        S, _ = check_case(G, sel, data, layouts(n, tile)["partial"], op=GT, threshold=threshold, items_are_stencil=True, form=LOCAL)
        assert 0 < S < n


@pytest.mark.parametrize("stencil,shift", [("float", 1), ("int", 2), ("uint", 3), ("double", 1)] + [("byte", s) for s in range(1, 16)])
def test_misaligned_bases(G, stencil, shift):
    """A stencil that starts `shift` elements behind a 16-byte boundary: tiles, waves and flag words are counted from that boundary,
    the boundaries from the array.  The items are shifted on their own, by one item."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    size = np.dtype(dtype).itemsize
    rng = np.random.default_rng(30 + shift)
    sel = G.Select()
    for n in (tile + 5, 2 * tile):
        data = as_stencil(flags_of("half", rng, n, tile, 1), dtype, rng)
        lay = layouts(n, tile)
        moved = u32(sorted({0, n} | {p - shift for p in lay["tile_edges"].tolist() if p >= shift}))  # the tile edges of the shifted base
        for offsets in (lay["per_element"], lay["tile_edges"], moved, lay["partial"]):
            for item_bytes, items_shift in ((4, 4), (8, 8), (16, 0)):
                check_case(G, sel, data, offsets, item_bytes=item_bytes, stencil_shift=shift * size, items_shift=items_shift, form=LOCAL)


@pytest.mark.parametrize("stencil", ["uint", "byte", "double"])
def test_overflow(G, stencil):
    """max_out at and below the number selected: the entries behind it are still poison, out_offsets is clamped to it and
    *num_selected is the true number (check_case expects all three)."""
    stencil_type, dtype = STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    rng = np.random.default_rng(20)
    n = 2 * tile + 9
    data = as_stencil(rng.integers(0, 3, n) == 0, dtype, rng)
    S = int((data != 0).sum())
    sel = G.Select()
    for max_out in (S, S - 1, S // 2, 1, 0):
        for name in ("tile_edges", "per_element"):
            got, out = check_case(G, sel, data, layouts(n, tile)[name], max_out=max_out, item_bytes=8, form=LOCAL)
            assert got == S and out.max() == out[-1] == max_out


def test_malformed_offsets(G):
    """Decreasing offsets, offsets beyond total and offsets that are all equal: everything except the LOCAL indices is what the
    definition says, and nothing outside the arrays is written."""
    tile = G.plan_select_batch(1, 1, 3)[0]
    rng = np.random.default_rng(40)
    n = 3 * tile + 17
    data = as_stencil(flags_of("half", rng, n, tile, 1), np.uint32, rng)
    sel = G.Select()
    good = np.sort(rng.integers(0, n + 1, 300)).astype(np.uint32)
    beyond = good.copy()
    beyond[150:] += np.uint32(2 * n)
    wild = good.copy()
    wild[7], wild[-1] = 0xFFFFFFFF, 0xFFFFFFF0
    ends_low = rng.permutation(good).astype(np.uint32)
    ends_low[0], ends_low[-1] = 10, n - 3  # a cover with shuffled boundaries inside
    cases = [(good[::-1].copy(), False), (rng.permutation(good).astype(np.uint32), False), (ends_low, False), (beyond, True), (wild, False),
             (np.full(300, tile + 1, dtype=np.uint32), True), (np.full(2, 0xFFFFFFFF, dtype=np.uint32), True),
             (rng.integers(0, 2**32, 300, dtype=np.uint32), False)]
    seen = 0
    for offsets, is_sorted in cases:
        for form in (GLOBAL, LOCAL):
            S, _ = check_case(G, sel, data, offsets, form=form, sorted_offsets=is_sorted)
            seen += S > 0
        check_case(G, sel, data, offsets, form=LOCAL, max_out=100, sorted_offsets=is_sorted)
    assert seen >= 6


def test_two_rounds_of_the_count_scan(G):
    """A byte stencil a little over 2^24 bytes: the plan says two rounds of the count scan.  One in 1000 selected plus the elements
    around the second round's first tile; boundaries on and around that tile, LOCAL indices and the offsets."""
    import torch

    B = G.SelectStencil_Byte
    n = (1 << 24) + 4099
    tile, tiles, rounds, kernels, _ = G.plan_select_batch(n, 9, B)
    assert rounds >= 2 and kernels == 4 and tile == 4096
    first = 4095 * tile  # count 4096 of the scan: the first of the second round
    mask = np.zeros(n, dtype=np.uint8)
    mask[::1000] = 1
    mask[[first - 1, first, first + tile - 1, first + tile, n - 1]] = 255
    offsets = u32([7, first - 1, first, first, first + 1, first + tile, n - tile, n - 1, n, n])
    idx, local, want_offsets, S = expected(mask != 0, offsets, n)
    max_out = S + 7
    mt, ft = torch.from_numpy(mask).cuda(), torch.from_numpy(offsets.view(np.int32)).cuda()
    ox, oo, na = Array.poisoned(max_out * 4), Array.poisoned(offsets.size * 4), Array.poisoned(4)
    G.Select().run_batch_offsets_ptr(mt.data_ptr(), n, ft.data_ptr(), offsets.size - 1, max_out, na.ptr, out_indices_ptr=ox.ptr,
                                     out_offsets_ptr=oo.ptr, index_form=LOCAL, stencil_type=B, stream=stream())
    torch.cuda.synchronize()
    assert int(na.result(np.uint32)[0]) == S
    assert (oo.result(np.uint32) == want_offsets).all()
    want = np.full(max_out, POISON32, dtype=np.uint32)
    want[:S] = local
    got = ox.result(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert (mt.cpu().numpy() == mask).all()
    del mt
    torch.cuda.empty_cache()


def test_argument_checks_and_overlaps(G):
    """One call per refusal the batched call adds to the single call's, and some of those it shares; a witness buffer (every output
    lies in it) shows that the refused calls wrote nothing."""
    import ctypes
    import torch

    sel = G.Select()
    n, parts = 4096, 8
    rng = np.random.default_rng(60)
    data = rng.integers(0, 2**32, n, dtype=np.uint32)
    st = torch.from_numpy(data.view(np.int32).copy()).cuda()
    it = torch.from_numpy(data.view(np.int32).copy()).cuda()
    ft = torch.from_numpy(np.arange(0, 64 * parts + 1, 64, dtype=np.int32)).cuda()
    wt = torch.zeros(4 * n, dtype=torch.int32, device="cuda")  # the witness: out_items, out_indices, num_selected, out_offsets
    sp, ip, fp, wp = st.data_ptr(), it.data_ptr(), ft.data_ptr(), wt.data_ptr()
    oi, ox, nu, oo = wp, wp + 4 * n, wp + 8 * n, wp + 12 * n
    U = G.SelectStencil_Uint

    def run(stencil=sp, total=512, offsets=fp, segments=parts, max_out=512, num=nu, indices=ox, items=ip, out_items=oi, item_bytes=4, out_offsets=oo,
            form=GLOBAL, stencil_type=U, op=NE):
        sel.run_batch_offsets_ptr(stencil, total, offsets, segments, max_out, num, indices, items, out_items, item_bytes, out_offsets, form,
                                  stencil_type, op)

    def equal(count=64, partitions=parts, **kw):
        sel.run_batch_ptr(sp, count, partitions, 512, nu, ox, ip, oi, 4, oo, kw.get("form", GLOBAL), U, NE)

    L, vp = G.lib(), ctypes.c_void_p
    bad = [
        (lambda: G.check(L.glu_select_run_batch_offsets_ptr(None, vp(sp), U, NE, None, 512, vp(fp), parts, None, 4, None, vp(ox), 0, 512, vp(oo),
                                                            vp(nu), None)), "select is NULL"),
        (lambda: G.check(L.glu_select_prepare_batch(None, 64, 2, U)), "select is NULL"),
        (lambda: run(stencil=None), "Invalid stencil buffer"),
        (lambda: run(num=None), "Invalid num_selected pointer"),
        (lambda: run(items=None), "items and out_items must both"),
        (lambda: run(stencil_type=13), "stencil_type"),
        (lambda: run(op=6), "op must be"),
        (lambda: run(item_bytes=12), "item_bytes must be"),
        (lambda: run(stencil=sp + 2), "stencil is not aligned"),
        (lambda: run(indices=ox + 2), "out_indices is not aligned"),
        (lambda: run(total=1 << 32), "fewer than 2^32"),
        (lambda: run(max_out=1 << 32), "max_out must be below 2^32"),
        (lambda: run(segments=(1 << 24) + 1), "exceeds 2^24"),
        (lambda: equal(count=1 << 20, partitions=1 << 12), "fewer than 2^32"),
        (lambda: equal(count=1 << 32, partitions=0), "count below 2^32"),
        (lambda: run(offsets=None), "Invalid offsets array"),
        (lambda: run(offsets=fp + 2), "offsets array is not aligned"),
        (lambda: run(out_offsets=oo + 2), "out_offsets is not aligned"),
        (lambda: run(form=2), "index_form must be"),
        (lambda: run(form=-1), "index_form must be"),
        (lambda: equal(form=7), "index_form must be"),
        (lambda: run(out_offsets=sp + 8), "out_offsets overlaps stencil"),
        (lambda: run(out_offsets=ip + 2044), "out_offsets overlaps items"),
        (lambda: run(out_offsets=fp + 4 * parts), "out_offsets overlaps offsets"),
        (lambda: run(out_offsets=oi + 2044), "out_offsets overlaps out_items"),
        (lambda: run(out_offsets=ox), "out_offsets overlaps out_indices"),
        (lambda: run(out_offsets=nu - 4 * parts), "out_offsets overlaps num_selected"),
        (lambda: run(out_items=fp), "out_items overlaps offsets"),
        (lambda: run(indices=fp + 4 * parts), "out_indices overlaps offsets"),
        (lambda: run(num=fp + 4), "num_selected overlaps offsets"),
        (lambda: sel.prepare_batch(1 << 32, 4), "fewer than 2^32"),
        (lambda: sel.prepare_batch(64, (1 << 24) + 1), "exceeds 2^24"),
        (lambda: sel.prepare_batch(64, 4, 5), "stencil_type"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    # arrays that only touch are fine: out_offsets ends where the offsets begin
    both = torch.from_numpy(np.concatenate([np.zeros(parts + 1, dtype=np.int32), np.arange(0, 64 * parts + 1, 64, dtype=np.int32)])).cuda()
    sel.run_batch_offsets_ptr(sp, 512, both.data_ptr() + 4 * (parts + 1), parts, 512, nu, out_offsets_ptr=both.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    want = expected(data[:512] != 0, np.arange(0, 64 * parts + 1, 64), 512)[2]
    assert (both.cpu().numpy().view(np.uint32)[:parts + 1] == want).all()


def test_prepared_captured_replayed(G):
    """After prepare_batch a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed
    on three other contents and other offsets of the same shape; a second run of the same input gives the same bytes."""
    import torch

    F = G.SelectStencil_Float
    tile = G.plan_select_batch(1, 1, F)[0]
    n, parts = 37 * tile + 11, 1000
    max_out = n // 4
    rng = np.random.default_rng(90)
    sel = G.Select()
    st = torch.empty(n, dtype=torch.float32, device="cuda")
    ft = torch.empty(parts + 1, dtype=torch.int32, device="cuda")
    oi = torch.empty(max_out, dtype=torch.int32, device="cuda")
    ox = torch.empty(max_out, dtype=torch.int32, device="cuda")
    oo = torch.empty(parts + 1, dtype=torch.int32, device="cuda")
    nt = torch.empty(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(data, offsets):
        st.copy_(torch.from_numpy(data))
        ft.copy_(torch.from_numpy(offsets.view(np.int32)))
        for t in (oi, ox, oo, nt):
            t.fill_(-1515870811)

    def outputs():
        return b"".join(t.cpu().numpy().tobytes() for t in (oi, ox, oo, nt))

    def verify(data, offsets):
        idx, local, want_offsets, S = expected(data > np.float32(0.5), offsets, max_out)
        m = min(S, max_out)
        assert int(nt.cpu().numpy().view(np.uint32)[0]) == S
        assert (oo.cpu().numpy().view(np.uint32) == want_offsets).all()
        want = np.full(max_out, POISON32, dtype=np.uint32)
        want[:m] = local[:m]
        assert (ox.cpu().numpy().view(np.uint32) == want).all()
        want[:m] = data[idx[:m]].view(np.uint32)
        assert (oi.cpu().numpy().view(np.uint32) == want).all()
        return S

    def call(s):
        sel.run_batch_offsets_ptr(st.data_ptr(), n, ft.data_ptr(), parts, max_out, nt.data_ptr(), ox.data_ptr(), st.data_ptr(), oi.data_ptr(), 4,
                                  oo.data_ptr(), LOCAL, F, GT, 0.5, s)

    def contents(share):  # uniform in [0, 1): above 0.5 with probability `share`; offsets with empty segments and a partial cover
        data = (rng.random(n, dtype=np.float32) * np.float32(0.5 / (1.0 - share))).astype(np.float32) if share < 0.5 else rng.random(n, dtype=np.float32)
        return data, np.sort(rng.integers(3, n - 3, parts + 1) // 7 * 7).astype(np.uint32)

    with torch.cuda.stream(side):
        data, offsets = contents(0.5)
        fill(data, offsets)
        side.synchronize()
        sel.prepare_batch(n, parts, F)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(data, offsets)
        first = outputs()
        fill(data, offsets)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert outputs() == first, "the same input gave other bytes"
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        seen = []
        for share in (0.5, 0.1, 0.001):
            data, offsets = contents(share)
            fill(data, offsets)
            graph.replay()
            side.synchronize()
            seen.append(verify(data, offsets))
        assert seen[0] > max_out > seen[1] > seen[2] > 0, (seen, max_out)


def test_with_the_family(G):
    """Sort 200 000 Zipf-keyed pairs, key runs, the batched select of the values above a threshold with out_offsets and LOCAL indices,
    the batched reduce of the compacted values over out_offsets -- four calls on one stream with no host read in between, against a
    numpy group-by: the sum of the kept values per group, zero for the groups that lost everything."""
    import torch

    rng = np.random.default_rng(70)
    n, max_runs = 200000, 4096
    keys = np.minimum(rng.zipf(1.3, n), 3000).astype(np.uint32) * np.uint32(7919)
    vals = rng.integers(0, 1000, n, dtype=np.uint32)
    threshold = 700
    kt, vt = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    offsets, runs_n = Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4)
    kept, local, kept_offsets, kept_n, sums = Array.poisoned(4 * n), Array.poisoned(4 * n), Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4), \
        Array.poisoned(4 * max_runs)
    s = stream()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "uint32", s)
    G.KeyRuns().run_ptr(kt.data_ptr(), n, offsets.ptr, max_runs, runs_n.ptr, stream=s)
    G.Select().run_batch_offsets_ptr(vt.data_ptr(), n, offsets.ptr, max_runs, n, kept_n.ptr, out_indices_ptr=local.ptr, items_ptr=vt.data_ptr(),
                                     out_items_ptr=kept.ptr, out_offsets_ptr=kept_offsets.ptr, index_form=LOCAL, op=GT, threshold=threshold, stream=s)
    G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum).run_batch_offsets_ptr(kept.ptr, sums.ptr, n, kept_offsets.ptr, max_runs, s)
    torch.cuda.synchronize()
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], vals[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    runs = heads.size
    assert int(runs_n.result(np.uint32)[0]) == runs and 1000 < runs < max_runs
    group = np.searchsorted(heads, np.arange(n), "right") - 1
    keep = sv > threshold
    want_sums = np.zeros(max_runs, dtype=np.uint64)
    np.add.at(want_sums, group[keep], sv[keep].astype(np.uint64))
    kept_per_group = np.bincount(group[keep], minlength=runs)
    assert (kept_per_group == 0).sum() > 10 and kept_per_group.max() > 1000  # groups that lost everything, and a long one
    assert int(kept_n.result(np.uint32)[0]) == int(keep.sum())
    got_offsets = kept_offsets.result(np.uint32)
    assert (got_offsets[:runs + 1] == np.concatenate([[0], np.cumsum(kept_per_group)])).all() and (got_offsets[runs:] == keep.sum()).all()
    assert (sums.result(np.uint32) == (want_sums & 0xFFFFFFFF).astype(np.uint32)).all()
    m = int(keep.sum())
    assert (kept.result(np.uint32)[:m] == sv[keep]).all() and (kept.result(np.uint32)[m:] == POISON32).all()
    idx = np.flatnonzero(keep)
    assert (local.result(np.uint32)[:m] == idx - heads[group[idx]]).all() and (local.result(np.uint32)[m:] == POISON32).all()


CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [%r, %r]
import test_gpu_select_batch as T
import glu_hip as G
import torch
before = G.scratch_filled_bytes()
digest, stated = hashlib.sha256(), 0
for stencil, total_tiles, shift in (("uint", 3, 0), ("byte", 2, 5), ("double", 1, 1)):
    stencil_type, dtype = T.STENCILS[stencil]
    tile = G.plan_select_batch(1, 1, stencil_type)[0]
    n = total_tiles * tile + 17
    rng = np.random.default_rng(total_tiles)
    data = T.as_stencil(T.flags_of("half", rng, n, tile, 1), dtype, rng)
    sel = G.Select()
    stated += G.plan_select_batch(n, 1, stencil_type)[4]
    for name in ("tile_edges", "partial", "per_element"):
        offsets = T.layouts(n, tile)[name]
        S, out = T.check_case(G, sel, data, offsets, form=T.LOCAL, item_bytes=8, stencil_shift=shift * np.dtype(dtype).itemsize)
        digest.update(out.tobytes() + bytes([S %% 251]))
    S, out = T.check_case(G, sel, data[:(n // 255) * 255], partition=255, form=T.LOCAL)
    digest.update(out.tobytes())
print("RESULT", digest.hexdigest(), G.scratch_filled_bytes() - before, stated)
"""


def run_child(fill):
    env = dict(os.environ)
    if fill is None:
        env.pop("GLU_HIP_SCRATCH_FILL", None)
    else:
        env["GLU_HIP_SCRATCH_FILL"] = fill
    code = CHILD % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gl-radix-sort_amd"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT"))
    _, digest, filled, stated = line.split()
    return digest, int(filled), int(stated)


@pytest.fixture(scope="module")
def unfilled(G):
    return run_child(None)


@pytest.mark.parametrize("fill", ["0x00", "0xFF", "0x5A"])
def test_no_result_depends_on_what_new_scratch_holds(G, unfilled, fill):
    """A handful of the cases above in a fresh process under GLU_HIP_SCRATCH_FILL: every output equals numpy's (check_case) and the
    offsets are the same bits as without a fill; the bytes filled are the scratch the plan states."""
    digest, filled, stated = run_child(fill)
    assert unfilled[1] == 0 and digest == unfilled[0]
    assert stated > 0 and filled == stated  # (the child makes Select objects only, one per stencil, and its first call is its largest)


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_select_batch_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
