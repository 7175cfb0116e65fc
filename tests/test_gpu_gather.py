"""GPU tests of gather and scatter (glu_gather_run_ptr, the two batched forms, glu_gather_scatter_ptr): items of 4, 8, 16 and 32
bytes fetched or placed by device indices.  The oracle is always numpy on the host (torch on the device for the one output beyond
4 GiB).  Every comparison is `==`.  Every array the call writes sits inside an allocation with 64 bytes of 0xA5 poison in front of
it and behind it, and is itself filled with poison first, so entries that must stay untouched are seen to stay untouched; the inputs
are checked unchanged.  The scheme is that of test_gpu_expand.py."""
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
GIB = 1 << 30
ITEM_SIZES = (4, 8, 16, 32)
BAD = np.array([2 ** 31, 2 ** 32 - 1], dtype=np.uint32)  # (with item_count and item_count + 1: the indices that are not trusted)


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

    def unchanged(self):
        return (self.t.cpu().numpy() == self.host).all()


def stream():
    """torch's current stream; where it is the default stream the handle is 0 and the library takes its own queue, which does not
    wait for torch's kernels: a test that makes an input with torch on the device calls sync() before it calls the library."""
    import torch

    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch

    torch.cuda.synchronize()


def tile_of(G, item_bytes):
    return G.plan_gather(1, item_bytes)[0]


def records(rng, n, item_bytes):
    """n items of random bytes, none of them all poison"""
    r = rng.integers(0, 256, (n, item_bytes), dtype=np.uint8)
    r[:, 0] &= 0x7F
    return r


def expect_tiles(G, g, count, item_bytes, first_byte):
    """last() is the plan's tiles, or one more where the streaming side starts inside a 16-byte pack"""
    tiles, kernels = g.last()
    if not count:
        assert (tiles, kernels) == (0, 0)
        return
    piece = min(item_bytes, 16)
    lo = (first_byte % 16) // piece
    T = tile_of(G, item_bytes)
    assert kernels == 1 and tiles == -(-(lo + count * (item_bytes // piece)) // (T * (item_bytes // piece))), (tiles, kernels, count, item_bytes)
    assert G.plan_gather(count, item_bytes)[1] <= tiles <= G.plan_gather(count, item_bytes)[1] + 1


def check_gather(G, g, items, idx, shifts=(0, 0, 0)):
    """One gather.  items: (item_count, item_bytes) uint8; idx: uint32.  shifts: bytes behind a 16-byte boundary of out, indices and
    items.  Returns the mask of the entries that were fetched."""
    item_count, item_bytes = items.shape
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    count = idx.size
    ib, xb, out = Array(items, shifts[2]), Array(idx, shifts[1]), Array.poisoned(count * item_bytes, shifts[0])
    g.run_ptr(ib.ptr, item_count, item_bytes, xb.ptr, count, out.ptr, stream())
    sync()
    what = (item_count, item_bytes, count, shifts)
    expect_tiles(G, g, count, item_bytes, out.ptr)
    valid = idx < item_count
    want = np.full((count, item_bytes), POISON, dtype=np.uint8)
    want[valid] = items[idx[valid]]
    got = out.result(np.uint8).reshape(count, item_bytes)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, int(bad[0]), int(idx[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())
    assert ib.unchanged() and xb.unchanged(), (what, "the call wrote to an input")
    return valid


def check_scatter(G, g, items, idx, out_count, shifts=(0, 0, 0)):
    """One scatter with DISTINCT valid indices.  shifts: of items (the streaming side), indices and out."""
    count, item_bytes = items.shape
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    ib, xb, out = Array(items, shifts[0]), Array(idx, shifts[1]), Array.poisoned(out_count * item_bytes, shifts[2])
    g.scatter_ptr(ib.ptr, item_bytes, xb.ptr, count, out.ptr, out_count, stream())
    sync()
    expect_tiles(G, g, count if out_count else 0, item_bytes, ib.ptr)
    valid = idx < out_count
    assert np.unique(idx[valid]).size == valid.sum()
    want = np.full((out_count, item_bytes), POISON, dtype=np.uint8)
    want[idx[valid]] = items[valid]
    got = out.result(np.uint8).reshape(out_count, item_bytes)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ((count, item_bytes, out_count, shifts), int(bad[0]))
    assert ib.unchanged() and xb.unchanged()
    return got


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_bytes", ITEM_SIZES)
def test_sizes(G, item_bytes):
    rng = np.random.default_rng(item_bytes)
    g = G.Gather()
    T, P = tile_of(G, item_bytes), max(1, 16 // item_bytes)
    items = records(rng, 1000, item_bytes)
    for count in sorted({0, 1, 2, 3, P - 1, P, P + 1, T - 1, T, T + 1, 3 * T + 5}):
        valid = check_gather(G, g, items, rng.integers(0, 1000, count))  # (duplicates: 3 T + 5 draws from 1000)
        assert valid.all()
    assert g.last() == (4, 1)


def test_alignment(G):
    """4-byte items with out and indices at every 4-byte step of a 16-byte period, independently; the wider items at every multiple
    of their alignment within 64 bytes (the indices and the items shifted too)."""
    rng = np.random.default_rng(50)
    g = G.Gather()
    for item_bytes in ITEM_SIZES:
        count = 2 * tile_of(G, item_bytes) + 3
        items = records(rng, 1000, item_bytes)
        idx = rng.integers(0, 1003, count).astype(np.uint32)  # (a few out of range: packs that go element by element)
        align = min(item_bytes, 16)
        if item_bytes == 4:
            for out_shift in (0, 4, 8, 12):
                for idx_shift in (0, 4, 8, 12):
                    check_gather(G, g, items, idx, (out_shift, idx_shift, (out_shift + idx_shift) % 16))
        else:
            for n, out_shift in enumerate(range(0, 64, align)):
                check_gather(G, g, items, idx, (out_shift, (4 * n) % 16, (align * n) % 16))
        for n, shift in enumerate(range(0, 64, align)):  # scatter: the streaming side is `items`
            perm = rng.permutation(count + 7).astype(np.uint32)[:count]
            check_scatter(G, g, records(rng, count, item_bytes), perm, count + 7, (shift, (4 * n) % 16, (align * (n + 1)) % 16))


# ---- indices that are not trusted -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [3, 100, 1])
@pytest.mark.parametrize("item_bytes", ITEM_SIZES)
def test_indices_are_not_trusted(G, item_bytes, rate):
    """item_count, item_count + 1, 2^31 and 2^32 - 1 among valid indices, one in `rate` (1: all of them): exactly those entries keep
    their poison (check_gather compares every entry, so the neighbours in the same pack are seen written)."""
    rng = np.random.default_rng(100 * item_bytes + rate)
    g = G.Gather()
    item_count, count = 777, 2 * tile_of(G, item_bytes) + 9
    items = records(rng, item_count, item_bytes)
    idx = rng.integers(0, item_count, count).astype(np.uint32)
    bad = rng.random(count) < 1.0 / rate
    idx[bad] = rng.choice(np.concatenate([BAD, np.array([item_count, item_count + 1], dtype=np.uint32)]), int(bad.sum()))
    valid = check_gather(G, g, items, idx, (8 if item_bytes <= 8 else 0, 4, 0))
    assert (valid == ~bad).all() and (bad.all() if rate == 1 else 0 < bad.sum() < count)


@pytest.mark.parametrize("item_bytes", ITEM_SIZES)
def test_shapes_of_index(G, item_bytes):
    rng = np.random.default_rng(7 + item_bytes)
    g = G.Gather()
    n = 3 * tile_of(G, item_bytes) + 1
    items = records(rng, n, item_bytes)
    iota = np.arange(n, dtype=np.uint32)
    for idx in (iota, iota[::-1], np.full(n, 5, dtype=np.uint32), rng.permutation(n), np.sort(rng.integers(0, n, n))):
        assert check_gather(G, g, items, idx).all()


# ---- scatter -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_bytes", ITEM_SIZES)
def test_scatter(G, item_bytes):
    rng = np.random.default_rng(300 + item_bytes)
    g = G.Gather()
    n = 3 * tile_of(G, item_bytes) + 5
    items = records(rng, n, item_bytes)
    perm = rng.permutation(n).astype(np.uint32)
    placed = check_scatter(G, g, items, perm, n)
    assert check_gather(G, g, placed, perm).all()  # ... and gather by the same indices returns the input (check_gather's oracle: placed[perm])
    assert (placed[perm] == items).all()
    # partial: count < out_count; what no index names keeps its poison (check_scatter's oracle)
    check_scatter(G, g, items[:n // 3], rng.permutation(n)[:n // 3], n, (min(item_bytes, 16) % 16, 4, 0))
    # indices out of range write nothing
    idx = perm.copy()
    out_of_range = rng.random(n) < 0.25
    idx[out_of_range] = rng.choice(np.concatenate([BAD, np.array([n, n + 1], dtype=np.uint32)]), int(out_of_range.sum()))
    check_scatter(G, g, items, idx, n)
    check_scatter(G, g, items, np.full(n, n, dtype=np.uint32) + np.arange(n, dtype=np.uint32), n)  # all of them
    for count, out_count in ((0, 10), (1, 1), (2, 5), (3, 3)):
        check_scatter(G, g, items[:count], rng.permutation(out_count)[:count], out_count)


@pytest.mark.parametrize("item_bytes", ITEM_SIZES)
def test_scatter_with_equal_indices(G, item_bytes):
    """Where indices are equal the entry holds one of the candidates; for 32-byte items each 16-byte half is one of the candidates'.
    Nothing else changes."""
    rng = np.random.default_rng(400 + item_bytes)
    g = G.Gather()
    count, out_count = 2 * tile_of(G, item_bytes) + 3, 97
    items = records(rng, count, item_bytes)
    idx = rng.integers(0, 60, count).astype(np.uint32)  # entries 60 .. 96 are named by no index
    ib, xb, out = Array(items), Array(idx), Array.poisoned(out_count * item_bytes)
    g.scatter_ptr(ib.ptr, item_bytes, xb.ptr, count, out.ptr, out_count, stream())
    sync()
    got = out.result(np.uint8).reshape(out_count, item_bytes)
    assert (got[60:] == POISON).all()
    piece = min(item_bytes, 16)
    for e in range(60):
        candidates = items[idx == e]
        assert candidates.shape[0] > 1
        for h in range(item_bytes // piece):
            half = got[e, h * piece:(h + 1) * piece]
            assert (candidates[:, h * piece:(h + 1) * piece] == half).all(axis=1).any(), (e, h)
    assert ib.unchanged() and xb.unchanged()


# ---- batched, on the real producer -----------------------------------------------------------------------------------------------------
def top_k_rows(keys, begin, end, k, largest, sorted_):
    """numpy's rows of batched top-k: per segment the local indices, k_s = min(k, length) of them"""
    rows = []
    for b, e in zip(begin, end):
        seg = keys[b:e]
        order = np.argsort(~seg if largest else seg, kind="stable")[:k]
        rows.append(order if sorted_ else np.sort(order))
    return rows


def check_batched(G, keys, k, offsets=None, count=0, largest=False, sorted_=True):
    """Batched top-k writes the rows of local indices; the batched gather fetches 8-byte records (low word: the key) through them."""
    rng = np.random.default_rng(k)
    total = keys.size
    recs = (rng.integers(0, 2 ** 32, total, dtype=np.uint64) << np.uint64(32)) | keys.astype(np.uint64)
    kb, rb = Array(keys), Array(recs)
    if offsets is None:
        n = total // count
        begin, end = np.arange(n) * count, (np.arange(n) + 1) * count
    else:
        n = offsets.size - 1
        begin, end = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
        fb = Array(offsets)
    ind, out = Array.poisoned(4 * n * k), Array.poisoned(8 * n * k, 8)
    topk, g = G.TopK(), G.Gather()
    if offsets is None:
        topk.run_batch_ptr(kb.ptr, count, n, k, None, ind.ptr, None, "uint32", largest, sorted_, stream())
        g.run_batch_ptr(rb.ptr, 8, count, n, ind.ptr, k, out.ptr, stream())
    else:
        topk.run_batch_offsets_ptr(kb.ptr, total, fb.ptr, n, k, None, ind.ptr, None, "uint32", largest, sorted_, stream())
        g.run_batch_offsets_ptr(rb.ptr, 8, total, fb.ptr, n, ind.ptr, k, out.ptr, stream())
    sync()
    expect_tiles(G, g, n * k, 8, out.ptr)
    want = np.full((n, k), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for s, row in enumerate(top_k_rows(keys, begin, end, k, largest, sorted_)):
        want[s, :row.size] = recs[begin[s] + row]
    got = out.result(np.uint64).reshape(n, k)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (k, n, bad[0].tolist())
    assert kb.unchanged() and rb.unchanged()


@pytest.mark.parametrize("k", [17, 1, 600])
def test_batched_equal_rows_from_top_k(G, k):
    rng = np.random.default_rng(500 + k)
    keys = rng.integers(0, 5000, 37 * 1000, dtype=np.uint32) * np.uint32(7919)  # (duplicates: ties by ascending index)
    check_batched(G, keys, k, count=1000, largest=False, sorted_=True)
    check_batched(G, keys, k, count=1000, largest=True, sorted_=False)


@pytest.mark.parametrize("k", [17, 1, 600])
def test_batched_offsets_from_top_k(G, k):
    """Empty segments, segments shorter than k, one segment of 5000: the entries behind k_s keep their poison."""
    rng = np.random.default_rng(600 + k)
    lens = np.array([0, 5, 0, 0, 16, 17, 18, 1, 5000, 0, 33, 599, 600, 601, 2, 0], dtype=np.int64)
    offsets = (np.concatenate([[0], np.cumsum(lens)]) + 3).astype(np.uint32)
    keys = rng.integers(0, 3000, int(offsets[-1]) + 6, dtype=np.uint32) * np.uint32(7919)
    check_batched(G, keys, k, offsets=offsets, largest=False, sorted_=True)
    check_batched(G, keys, k, offsets=offsets, largest=True, sorted_=False)


def test_batched_malformed_offsets_write_nothing_for_those_segments(G):
    """A decreasing pair and an end beyond total: those segments are empty.  The items end where their allocation ends, and every
    index is in range of a well-formed neighbour, so a segment taken at its word would be seen in `out`."""
    import torch

    rng = np.random.default_rng(77)
    g = G.Gather()
    lens = np.array([40, 50, 60, 70, 80, 90], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total, n, k = int(offsets[-1]), lens.size, 23
    offsets[3] = offsets[2] - 7  # segment 2 ends below its begin (empty); segment 3 is [offsets[2] - 7, offsets[4]), 137 long
    offsets[-1] = total + 1  # the last segment ends beyond total (empty)
    for item_bytes in ITEM_SIZES:
        items = records(rng, total, item_bytes)
        room = torch.full((4096 + total * item_bytes,), POISON, dtype=torch.uint8, device="cuda")
        room[4096:] = torch.from_numpy(items.reshape(-1)).cuda()  # the items end with the allocation
        idx = rng.integers(0, 40, n * k).astype(np.uint32)
        fb, xb, out = Array(offsets), Array(idx), Array.poisoned(n * k * item_bytes)
        g.run_batch_offsets_ptr(room.data_ptr() + 4096, item_bytes, total, fb.ptr, n, xb.ptr, k, out.ptr, stream())
        sync()
        begin, end = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
        end = np.where((end < begin) | (end > total), begin, end)
        assert (end - begin).tolist() == [40, 50, 0, 137, 80, 0]
        want = np.full((n, k, item_bytes), POISON, dtype=np.uint8)
        for s in range(n):
            for j in range(min(k, end[s] - begin[s])):
                if idx[s * k + j] < end[s] - begin[s]:
                    want[s, j] = items[begin[s] + idx[s * k + j]]
        assert (out.result(np.uint8).reshape(n, k, item_bytes) == want).all(), item_bytes
        assert (room.cpu().numpy()[4096:].reshape(total, item_bytes) == items).all() and fb.unchanged() and xb.unchanged()
    # indices not below the segment's length, in a row of equal partitions: those entries alone keep their poison
    count, parts, k = 50, 9, 60  # k > count: the entries behind k_s = 50 of every row stay too
    items = records(rng, count * parts, 16)
    idx = rng.integers(0, 55, parts * k).astype(np.uint32)
    ib, xb, out = Array(items), Array(idx), Array.poisoned(parts * k * 16)
    g.run_batch_ptr(ib.ptr, 16, count, parts, xb.ptr, k, out.ptr, stream())
    sync()
    want = np.full((parts, k, 16), POISON, dtype=np.uint8)
    for s in range(parts):
        for j in range(count):
            if idx[s * k + j] < count:
                want[s, j] = items[s * count + idx[s * k + j]]
    assert (out.result(np.uint8).reshape(parts, k, 16) == want).all()


# ---- wide addresses ------------------------------------------------------------------------------------------------------------------
def need(nbytes):
    """Skips unless `nbytes` and 2 GiB more are free."""
    import torch

    assert nbytes <= 40 * GIB, "no test may need more than 40 GiB"
    if torch.cuda.mem_get_info()[0] < nbytes + 2 * GIB:
        pytest.skip("needs %d GiB of free HBM" % -(-nbytes // GIB))


def release():
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


def zones(rng, n, middle, how_many=10000):
    """`how_many` indices, with duplicates, from the first 2048, the last 2048 and the 4096 around `middle` of [0, n)"""
    pool = np.concatenate([np.arange(2048), np.arange(middle - 2048, middle + 2048), np.arange(n - 2048, n)]).astype(np.int64)
    return rng.choice(pool, how_many), pool


def wide_gather(G, item_bytes, item_count, middle):
    """The table is allocated whole; only the items that are read are ever written."""
    import torch

    need(item_count * item_bytes + GIB)
    rng = np.random.default_rng(item_bytes)
    words = item_bytes // 4
    idx, pool = zones(rng, item_count, middle)
    values = rng.integers(0, 2 ** 31, (pool.size, words), dtype=np.int64).astype(np.int32)
    table = torch.empty((item_count, words), dtype=torch.int32, device="cuda")
    table[torch.from_numpy(pool).cuda()] = torch.from_numpy(values).cuda()
    xb, out = Array(idx.astype(np.uint32)), Array.poisoned(idx.size * item_bytes)
    g = G.Gather()
    sync()
    g.run_ptr(table.data_ptr(), item_count, item_bytes, xb.ptr, idx.size, out.ptr, stream())
    sync()
    want = values[np.searchsorted(pool, idx)]
    assert (out.result(np.int32).reshape(idx.size, words) == want).all()
    del table
    release()


def test_wide_byte_offsets_past_4_gib(G):
    wide_gather(G, 16, 2 ** 28 + 4096, 2 ** 28)


def test_wide_index_sign_bit(G):
    wide_gather(G, 4, 2 ** 31 + 4096, 2 ** 31)


def test_wide_scatter_past_4_gib(G):
    import torch

    out_count, middle = 2 ** 27 + 4096, 2 ** 27
    need(out_count * 32 + GIB)
    rng = np.random.default_rng(32)
    _, pool = zones(rng, out_count, middle)
    idx = rng.permutation(pool)[:5000]  # distinct
    items = rng.integers(0, 2 ** 31, (idx.size, 8), dtype=np.int64).astype(np.int32)
    out = torch.empty((out_count, 8), dtype=torch.int32, device="cuda")
    where = torch.from_numpy(pool).cuda()
    out[where] = -1515870811  # poison in the zones that are looked at
    ib, xb = Array(items), Array(idx.astype(np.uint32))
    g = G.Gather()
    sync()
    g.scatter_ptr(ib.ptr, 32, xb.ptr, idx.size, out.data_ptr(), out_count, stream())
    sync()
    want = np.full((pool.size, 8), -1515870811, dtype=np.int32)
    want[np.searchsorted(pool, idx)] = items
    assert (out[where].cpu().numpy() == want).all()
    assert ib.unchanged() and xb.unchanged()
    del out
    release()


def test_wide_out_past_4_gib(G):
    """count = 2^30 + 4099 outputs of 4 bytes from a table of 2^16 items; the indices are made on the device.  The first and the last
    outputs and the two 64 KiB chunks around the 4 GiB line are compared with torch on the device."""
    import torch

    count, guard = 2 ** 30 + 4099, 16
    need(2 * 4 * count + GIB)
    table = torch.randint(0, 2 ** 31 - 1, (2 ** 16,), dtype=torch.int32, device="cuda")
    idx = torch.empty(count, dtype=torch.int32, device="cuda")
    step = 2 ** 26
    for a in range(0, count, step):
        b = min(count, a + step)
        idx[a:b] = (((torch.arange(a, b, dtype=torch.int64, device="cuda") * 2654435761) >> 9) & 0xFFFF).to(torch.int32)
    room = torch.full((count + 2 * guard,), -1515870811, dtype=torch.int32, device="cuda")
    out = room[guard:guard + count]
    g = G.Gather()
    sync()
    g.run_ptr(table.data_ptr(), 2 ** 16, 4, idx.data_ptr(), count, out.data_ptr(), stream())
    sync()
    assert g.last() == G.plan_gather(count, 4)[1:3]
    line = 2 ** 30  # the output whose byte offset is 4 GiB
    for a, b in ((0, 16384), (line - 16384, line), (line, line + 16384), (count - 16384, count)):
        assert torch.equal(out[a:b], table[idx[a:b].long()]), (a, b)
    assert (room[:guard] == -1515870811).all().item() and (room[guard + count:] == -1515870811).all().item()
    del room, out, idx
    release()


# ---- captured and replayed ------------------------------------------------------------------------------------------------------------
def test_captured_replayed(G):
    """One gather and one batched-offsets gather, captured on a side stream as a linear chain, are replayed on three contents of the
    same sizes: the launch sequence does not depend on the data.  The calls leave the device's free memory as they found it."""
    import torch

    rng = np.random.default_rng(90)
    g = G.Gather()
    T = tile_of(G, 8)
    item_count, count, n, k = 5000, 5 * T + 3, 40, 13
    it = torch.empty(item_count, dtype=torch.int64, device="cuda")
    xt = torch.empty(count, dtype=torch.int32, device="cuda")
    ft = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    rt = torch.empty(n * k, dtype=torch.int32, device="cuda")
    out, rows = torch.empty(count, dtype=torch.int64, device="cuda"), torch.empty(n * k, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def content(seed):
        r = np.random.default_rng(seed)
        items = r.integers(0, 2 ** 62, item_count, dtype=np.int64)
        idx = r.integers(0, item_count + (item_count // 10) * seed, count).astype(np.uint32)  # (seed 0: all in range)
        lens = r.multinomial(item_count - 9, np.ones(n) / n) * (r.integers(0, 3, n) > 0)
        offsets = (np.concatenate([[0], np.cumsum(lens)]) + 4).astype(np.uint32)
        ridx = r.integers(0, 140, n * k).astype(np.uint32)
        return items, idx, offsets, ridx

    def fill(c):
        items, idx, offsets, ridx = c
        for t, a in ((it, items), (xt, idx.view(np.int32)), (ft, offsets.view(np.int32)), (rt, ridx.view(np.int32))):
            t.copy_(torch.from_numpy(a))
        out.fill_(-1)
        rows.fill_(-1)

    def verify(c):
        items, idx, offsets, ridx = c
        want = np.full(count, -1, dtype=np.int64)
        want[idx < item_count] = items[idx[idx < item_count]]
        assert (out.cpu().numpy() == want).all()
        want = np.full((n, k), -1, dtype=np.int64)
        for s in range(n):
            length = int(offsets[s + 1]) - int(offsets[s])
            for j in range(min(k, length)):
                if ridx[s * k + j] < length:
                    want[s, j] = items[offsets[s] + ridx[s * k + j]]
        assert (rows.cpu().numpy().reshape(n, k) == want).all()

    def call(s):
        g.run_ptr(it.data_ptr(), item_count, 8, xt.data_ptr(), count, out.data_ptr(), s)
        g.run_batch_offsets_ptr(it.data_ptr(), 8, item_count, ft.data_ptr(), n, rt.data_ptr(), k, rows.data_ptr(), s)

    contents = [content(seed) for seed in (0, 1, 2)]
    with torch.cuda.stream(side):
        fill(contents[0])
        side.synchronize()
        G.Gather().run_ptr(it.data_ptr(), item_count, 8, xt.data_ptr(), count, out.data_ptr(), side.cuda_stream)  # (loads the kernels)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)  # (the first calls of this object: no scratch, no prepare)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a call changed the device memory in use"
        verify(contents[0])
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for c in contents[::-1]:
            fill(c)
            graph.replay()
            side.synchronize()
            verify(c)


# ---- with the family -----------------------------------------------------------------------------------------------------------------
def test_stable_sort_of_wide_records(G):
    """The stable sort of 32-byte records by a float32 key: sort the keys beside an iota, then gather the records through it."""
    rng = np.random.default_rng(800)
    n = 50001
    keys = rng.integers(-300, 300, n).astype(np.float32) / np.float32(4)  # (duplicates: stable by index)
    recs = records(rng, n, 32)
    kb, vb, rb, out = Array(keys), Array(np.arange(n, dtype=np.uint32)), Array(recs), Array.poisoned(32 * n)
    G.RadixSort().sort_typed_ptr(kb.ptr, vb.ptr, n, "float32", stream())
    G.Gather().run_ptr(rb.ptr, n, 32, vb.ptr, n, out.ptr, stream())
    sync()
    bits = keys.view(np.uint32)
    code = np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000))  # the sort's order of floats: by their bits
    order = np.argsort(code, kind="stable")
    assert (vb.result(np.uint32) == order).all()
    assert (out.result(np.uint8).reshape(n, 32) == recs[order]).all()


def test_the_values_at_a_top_k(G):
    rng = np.random.default_rng(801)
    n, k = 100003, 257
    keys = rng.integers(0, 30000, n, dtype=np.uint32)
    vals = records(rng, n, 16)
    kb, vb, ind, out = Array(keys), Array(vals), Array.poisoned(4 * k), Array.poisoned(16 * k)
    G.TopK().run_ptr(kb.ptr, n, k, None, ind.ptr, None, "uint32", True, True, stream())
    G.Gather().run_ptr(vb.ptr, n, 16, ind.ptr, k, out.ptr, stream())
    sync()
    order = np.argsort(~keys, kind="stable")[:k]
    assert (out.result(np.uint8).reshape(k, 16) == vals[order]).all()


def test_select_gather_add_one_scatter_back(G):
    """Select's indices, gather, add one, scatter back: numpy's masked update."""
    import torch

    rng = np.random.default_rng(802)
    n = 100003
    d = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    want_idx = np.flatnonzero(d > np.uint32(0xC0000000))
    m = want_idx.size
    db, ib, nb = Array(d), Array.poisoned(4 * (m + 50)), Array.poisoned(4)
    picked = torch.full((m,), -1515870811, dtype=torch.int32, device="cuda")
    g = G.Gather()
    sync()
    G.Select().run_ptr(db.ptr, n, m + 50, nb.ptr, out_indices_ptr=ib.ptr, stencil_type=G.SelectStencil_Uint, op=G.SelectOperator_GT,
                       threshold=0xC0000000, stream=stream())
    g.run_ptr(db.ptr, n, 4, ib.ptr, m, picked.data_ptr(), stream())
    sync()
    picked += 1
    sync()
    g.scatter_ptr(picked.data_ptr(), 4, ib.ptr, m, db.ptr, n, stream())
    sync()
    assert int(nb.result(np.uint32)[0]) == m and 0 < m < n
    want = d.copy()
    want[want_idx] += np.uint32(1)
    assert (db.result(np.uint32) == want).all()


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(G):
    """Every refusal of the contract: INVALID_ARGUMENT with a message that names the argument, and a witness buffer (every output
    lies in it) shows that nothing was written."""
    import torch

    g = G.Gather()
    n, count, segs, k = 1024, 512, 8, 16
    far = 8 * n  # words between the arrays of the input allocation
    it = torch.zeros(4 * far, dtype=torch.int32, device="cuda")  # items, then indices, then offsets, `far` words apart
    it[2 * far:2 * far + segs + 1] = torch.arange(0, n + 1, n // segs, dtype=torch.int32, device="cuda")
    wt = torch.zeros(16 * n, dtype=torch.int32, device="cuda")  # the witness: out
    ip, xp, fp, op = it.data_ptr(), it.data_ptr() + 4 * far, it.data_ptr() + 8 * far, wt.data_ptr()
    L, vp = G.lib(), ctypes.c_void_p

    def run(items=ip, item_count=n, item_bytes=4, idx=xp, count_=count, out=op):
        g.run_ptr(items, item_count, item_bytes, idx, count_, out)

    def scatter(items=ip, item_bytes=4, idx=xp, count_=count, out=op, out_count=n):
        g.scatter_ptr(items, item_bytes, idx, count_, out, out_count)

    def parts(items=ip, item_bytes=4, count_=n // segs, num=segs, idx=xp, k_=k, out=op):
        g.run_batch_ptr(items, item_bytes, count_, num, idx, k_, out)

    def offs(items=ip, item_bytes=4, total=n, offsets=fp, num=segs, idx=xp, k_=k, out=op):
        g.run_batch_offsets_ptr(items, item_bytes, total, offsets, num, idx, k_, out)

    bad = [
        (lambda: G.check(L.glu_gather_run_ptr(None, vp(ip), n, 4, vp(xp), count, vp(op), None)), "gather is NULL"),
        (lambda: G.check(L.glu_gather_run_batch_ptr(None, vp(ip), 4, n // segs, segs, vp(xp), k, vp(op), None)), "gather is NULL"),
        (lambda: G.check(L.glu_gather_run_batch_offsets_ptr(None, vp(ip), 4, n, vp(fp), segs, vp(xp), k, vp(op), None)), "gather is NULL"),
        (lambda: G.check(L.glu_gather_scatter_ptr(None, vp(ip), 4, vp(xp), count, vp(op), n, None)), "gather is NULL"),
        (lambda: G.check(L.glu_gather_last(None, None, None)), "gather is NULL"),
        (lambda: G.check(L.glu_gather_create(None)), "out is NULL"),
        (lambda: run(items=None), "items is NULL"),
        (lambda: run(idx=None), "indices is NULL"),
        (lambda: run(out=None), "out is NULL"),
        (lambda: scatter(items=None), "items is NULL"),
        (lambda: scatter(idx=None), "indices is NULL"),
        (lambda: scatter(out=None), "out is NULL"),
        (lambda: parts(items=None), "items is NULL"),
        (lambda: parts(idx=None), "indices is NULL"),
        (lambda: offs(out=None), "out is NULL"),
        (lambda: offs(offsets=None), "offsets is NULL"),
        (lambda: run(item_bytes=0), "item_bytes must be 4, 8, 16 or 32"),
        (lambda: run(item_bytes=12), "item_bytes must be 4, 8, 16 or 32"),
        (lambda: scatter(item_bytes=64), "item_bytes must be 4, 8, 16 or 32"),
        (lambda: parts(item_bytes=2), "item_bytes must be 4, 8, 16 or 32"),
        (lambda: offs(item_bytes=24), "item_bytes must be 4, 8, 16 or 32"),
        (lambda: run(items=ip + 2), "items is not aligned to 4 bytes"),
        (lambda: run(items=ip + 4, item_bytes=8), "items is not aligned to 8 bytes"),
        (lambda: run(items=ip + 8, item_bytes=32), "items is not aligned to 16 bytes"),
        (lambda: run(out=op + 8, item_bytes=16), "out is not aligned to 16 bytes"),
        (lambda: run(idx=xp + 2), "indices is not aligned to 4 bytes"),
        (lambda: scatter(items=ip + 4, item_bytes=8), "items is not aligned to 8 bytes"),
        (lambda: scatter(out=op + 4, item_bytes=16), "out is not aligned to 16 bytes"),
        (lambda: scatter(idx=xp + 1), "indices is not aligned to 4 bytes"),
        (lambda: parts(out=op + 2), "out is not aligned to 4 bytes"),
        (lambda: offs(offsets=fp + 2), "offsets is not aligned to 4 bytes"),
        (lambda: offs(idx=xp + 3), "indices is not aligned to 4 bytes"),
        (lambda: run(count_=2 ** 32), "count must be below 2^32"),
        (lambda: run(item_count=2 ** 32 + 1), "item_count must not exceed 2^32"),
        (lambda: scatter(count_=2 ** 32), "count must be below 2^32"),
        (lambda: scatter(out_count=2 ** 32 + 1), "out_count must not exceed 2^32"),
        (lambda: offs(num=2 ** 24 + 1), "num_segments"),
        (lambda: offs(total=2 ** 32), "a batch must hold fewer than 2^32 elements"),
        (lambda: offs(num=2 ** 20, k_=2 ** 12), "num_segments * k must stay below 2^32"),
        (lambda: parts(count_=2 ** 20, num=2 ** 12), "a batch must hold fewer than 2^32 elements"),
        (lambda: parts(count_=2 ** 40, num=2 ** 24), "count * num_partitions overflows"),
        (lambda: parts(count_=16, num=2 ** 10, k_=2 ** 22), "num_segments * k must stay below 2^32"),
        (lambda: run(out=ip), "out overlaps items"),
        (lambda: run(out=ip + 4 * (n - 1)), "out overlaps items"),
        (lambda: run(out=xp - 4 * (count - 1)), "out overlaps indices"),
        (lambda: scatter(out=ip + 4 * (count - 1)), "out overlaps items"),
        (lambda: scatter(out=xp - 4 * (n - 1)), "out overlaps indices"),
        (lambda: parts(out=ip), "out overlaps items"),
        (lambda: parts(out=xp + 4 * (segs * k - 1)), "out overlaps indices"),
        (lambda: offs(out=fp + 4 * segs), "out overlaps offsets"),
        (lambda: offs(out=fp - 4 * (segs * k - 1)), "out overlaps offsets"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    sync()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    # nothing to do: GLU_OK, nothing enqueued, no array looked at
    for call in (lambda: run(items=None, idx=None, out=None, count_=0), lambda: run(items=None, idx=None, out=None, item_count=0),
                 lambda: scatter(items=None, idx=None, out=None, count_=0), lambda: scatter(items=None, idx=None, out=None, out_count=0),
                 lambda: parts(items=None, idx=None, out=None, k_=0), lambda: parts(items=None, idx=None, out=None, num=0),
                 lambda: offs(items=None, idx=None, out=None, offsets=None, k_=0), lambda: offs(items=None, idx=None, out=None, offsets=None, num=0)):
        run()
        assert g.last() == (1, 1)
        call()
        assert g.last() == (0, 0)
    # arrays that only touch are fine: the indices, then out right behind them, the items right behind out
    big = torch.zeros(3 * count, dtype=torch.int32, device="cuda")
    big[:count] = torch.arange(count - 1, -1, -1, dtype=torch.int32, device="cuda")
    big[2 * count:] = torch.arange(count, dtype=torch.int32, device="cuda") * 3
    bp = big.data_ptr()
    sync()
    g.run_ptr(bp + 8 * count, count, 4, bp, count, bp + 4 * count, stream())
    sync()
    assert (big[count:2 * count].cpu().numpy() == np.arange(count - 1, -1, -1) * 3).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_gather_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
