"""GPU tests of the batched sorted search (glu_sorted_search_run_batch_ptr, glu_sorted_search_run_batch_offsets_ptr): every
segment's needles in that segment's own haystack.  Expected values are always numpy.searchsorted(enc(hay[hb:he]), enc(needles[nb:ne]),
side) per segment on the keys as the sort encodes them, compared with `==`; a needle that belongs to no segment keeps its poison.
Every array the call reads or writes sits inside an allocation with poison in front of it and behind it, the outputs are filled with
poison first, the inputs are checked unchanged and last() is held against the plan.  Offsets are always well-formed here; malformed
ones are tests/test_search_batch_walk.py's.  The scheme is that of test_gpu_sorted_search.py."""
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
BATCH = 3
DEFAULT = 0xFFFFFFFF
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
GIB = 1 << 30


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
    import torch

    return torch.cuda.current_stream().cuda_stream


def enc(a):
    """The sort's encoding of an array of one of the six key types: unsigned keys in the sort's order."""
    a = np.ascontiguousarray(a)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    bits = a.view(u)
    sign = u(1) << u(8 * a.dtype.itemsize - 1)
    if a.dtype.kind == "u":
        return bits.copy()
    if a.dtype.kind == "i":
        return bits ^ sign
    return np.where(bits & sign != 0, ~bits, bits | sign)


def offsets_of(lengths, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]) + first).astype(np.uint32)


def expected(hay, hay_offsets, needles, needle_offsets):
    """(lower, upper) per segment on the encoded keys; poison where a needle belongs to no segment."""
    eh, en = enc(hay), enc(needles)
    lower, upper = np.full(needles.size, POISON32, dtype=np.uint32), np.full(needles.size, POISON32, dtype=np.uint32)
    ho, no = hay_offsets.astype(np.int64), needle_offsets.astype(np.int64)
    assert (np.diff(ho) >= 0).all() and (np.diff(no) >= 0).all() and ho[-1] <= hay.size and no[-1] <= needles.size
    for s in np.flatnonzero(np.diff(no)):
        h, n = eh[ho[s]:ho[s + 1]], en[no[s]:no[s + 1]]
        assert (h[1:] >= h[:-1]).all(), "the test's haystack is not sorted"
        lower[no[s]:no[s + 1]] = np.searchsorted(h, n, "left")
        upper[no[s]:no[s + 1]] = np.searchsorted(h, n, "right")
    return lower, upper


def check_batch(G, ss, hay, needles, hay_offsets=None, needle_offsets=None, rows=None, outputs="both", window=None, shifts=(0, 0, 0),
                want=None):
    """One call.  rows = (num_partitions, hay_count, needle_count): equal partitions; else the offsets form, needle_offsets None for
    equal needle rows.  Every output compared with `==`, the poison around all the arrays checked, the inputs unchanged, last() as the
    plan says.  Returns (lower, upper) as numpy gives them."""
    import torch

    key_type = str(hay.dtype)
    ha, na = Array(hay, shifts[0]), Array(needles, shifts[1])
    lo, up = Array.poisoned(4 * needles.size, shifts[2]), Array.poisoned(4 * needles.size, shifts[2])
    lo_ptr, up_ptr = lo.ptr if outputs in ("both", "lower") else None, up.ptr if outputs in ("both", "upper") else None
    if window is not None:
        ss.set_batch_window(window)
    inputs = [ha, na]
    if rows is not None:
        P, n, m = rows
        assert hay.size == P * n and needles.size == P * m
        ss.run_batch_ptr(ha.ptr, n, na.ptr, m, P, lo_ptr, up_ptr, key_type, stream())
        ho, no = np.arange(P + 1, dtype=np.int64) * n, np.arange(P + 1, dtype=np.int64) * m
    else:
        S = hay_offsets.size - 1
        hoa = Array(hay_offsets.astype(np.uint32))
        noa = Array(needle_offsets.astype(np.uint32)) if needle_offsets is not None else None
        inputs += [hoa] + ([noa] if noa else [])
        ss.run_batch_offsets_ptr(ha.ptr, hay.size, hoa.ptr, na.ptr, needles.size, noa.ptr if noa else None, S, lo_ptr, up_ptr, key_type, stream())
        ho = hay_offsets
        no = needle_offsets if needle_offsets is not None else np.arange(S + 1, dtype=np.int64) * (needles.size // S)
    torch.cuda.synchronize()
    what = (key_type, hay.size, needles.size, rows, outputs, window, shifts)
    assert ss.last() == (BATCH, 0, G.plan_sorted_search_batch(needles.size, key_type, 0)[3]), (what, ss.last())
    want = want or expected(hay, np.asarray(ho), needles, np.asarray(no))
    for name, arr, w in (("lower", lo, want[0]), ("upper", up, want[1])):
        got = arr.result(np.uint32)
        if outputs not in ("both", name):
            w = np.full(needles.size, POISON32, dtype=np.uint32)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, (what, name, bad.size, int(bad[0]), int(got[bad[0]]), int(w[bad[0]]))
    for a in inputs:
        assert a.unchanged(), "the call wrote to an input or around it"
    return want


def keys_of(ints, dtype):
    """Small integers as keys of `dtype`: negative and fractional values for the signed and the float types; the numeric order of
    these values is the sort's order."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return ints.astype(dtype)
    if dtype.kind == "i":
        return (ints.astype(np.int64) - 100).astype(dtype)
    return ((ints.astype(np.float64) - 100) / 4).astype(dtype)


def sorted_rows(rng, offsets, span, dtype, disjoint=False):
    """Keys sorted inside every segment.  All segments draw from the same range [0, span), so that a probe that leaks into a
    neighbouring segment changes the answer; `disjoint`: segment s draws from [s * span, (s + 1) * span)."""
    total = int(offsets[-1])
    ints = rng.integers(0, span, total)
    for s, (b, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        ints[b:e] = np.sort(ints[b:e]) + (s * span if disjoint else 0)
    return keys_of(ints, dtype)


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_equal_rows_whose_tiles_straddle_rows(G, key_type):
    """37 rows x (128 keys, 100 needles): a tile of 2048 or 1024 needles holds 20 or 10 rows and ends inside one.  Neighbouring rows
    hold the same key range; a second run holds disjoint ranges.  Every byte shift the key size allows."""
    rng = np.random.default_rng(37)
    P, n, m = 37, 128, 100
    kb = np.dtype(key_type).itemsize
    ss = G.SortedSearch()
    for disjoint in (False, True):
        hay = sorted_rows(rng, np.arange(P + 1) * n, 300, key_type, disjoint)
        # (disjoint: a row's needles come from its own range and from both neighbours')
        needles = keys_of(np.maximum(rng.integers(-300, 602, P * m) + np.repeat(np.arange(P), m) * 300, 0) if disjoint
                          else rng.integers(0, 302, P * m), key_type)
        want = None
        for outputs in ("both", "lower", "upper"):
            for shift in (0, 4, 8, 12):
                key_shift = shift if shift % kb == 0 else (shift + 4) % 16
                want = check_batch(G, ss, hay, needles, rows=(P, n, m), outputs=outputs, shifts=(key_shift, (key_shift + 8) % 16, shift),
                                   want=want)
        assert (want[1] > want[0]).sum() > (100 if disjoint else 500) and (want[0] == want[1]).sum() > 100  # present and absent needles
        if not disjoint:
            assert want[0].max() <= n and (want[1] == n).any() and (want[0] == 0).any()


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_rows_longer_than_a_tile_at_every_window(G, key_type):
    """3 rows x (5000, 5000): the default window holds a row (8192 keys) or not (4096 8-byte keys); 4096 sends these rows to
    global memory; 0 never stages.  All give the same outputs."""
    rng = np.random.default_rng(5000)
    P, n, m = 3, 5000, 5000
    hay = sorted_rows(rng, np.arange(P + 1) * n, 9000, key_type)
    needles = keys_of(rng.integers(0, 9002, P * m), key_type)
    ss = G.SortedSearch()
    want = None
    for window in (DEFAULT, 4096, 0):
        want = check_batch(G, ss, hay, needles, rows=(P, n, m), window=window, want=want, shifts=(0, 8, 4))


@pytest.mark.parametrize("n", [4096, 4097])
def test_the_window_edge_at_the_default(G, n):
    """8-byte keys, whose default window is 4096 keys: rows of 4096 keys with one tile of 1024 needles each fill the window exactly;
    rows of 4097 keys are one key over."""
    rng = np.random.default_rng(n)
    P, m = 3, 1024
    assert G.plan_sorted_search_batch(P * m, "uint64")[:3] == (1024, 3, 4096)
    hay = sorted_rows(rng, np.arange(P + 1) * n, 5000, "uint64")
    needles = keys_of(rng.integers(0, 5002, P * m), "uint64")
    needles[::m], needles[1::m] = 0, 5001  # in every row: not above its first key, above its last
    ss = G.SortedSearch()
    want = check_batch(G, ss, hay, needles, rows=(P, n, m))
    check_batch(G, ss, hay, needles, rows=(P, n, m), window=0, want=want)
    assert (want[1] == n).any() and (want[0] == 0).any()


@pytest.mark.parametrize("per_row", [51, 52, 53])
def test_the_window_edge_at_a_small_window(G, per_row):
    """4-byte keys, window 256.  Five segments whose haystacks make 255, 256 (+ 4 keys of slack taken from the first) and 257 keys
    under one tile of 2048 needles; then 16 rows of 128 keys under one tile: more rows than the window holds."""
    rng = np.random.default_rng(per_row)
    lengths = np.full(5, per_row)
    lengths[0] -= {51: 0, 52: 4, 53: 8}[per_row]  # 255, 256, 257 keys
    assert lengths.sum() == {51: 255, 52: 256, 53: 257}[per_row]
    ho, no = offsets_of(lengths), offsets_of([400, 17, 800, 0, 831])
    assert no[-1] == 2048
    hay = sorted_rows(rng, ho, 90, "uint32")
    needles = keys_of(rng.integers(0, 92, 2048), "uint32")
    ss = G.SortedSearch()
    want = check_batch(G, ss, hay, needles, ho, no, window=256)
    check_batch(G, ss, hay, needles, ho, no, window=0, want=want)
    check_batch(G, ss, hay, needles, ho, no, window=DEFAULT, want=want)
    hay = sorted_rows(rng, np.arange(17) * 128, 300, "int32")
    needles = keys_of(rng.integers(0, 302, 2048), "int32")
    want = check_batch(G, ss, hay, needles, rows=(16, 128, 128), window=256)
    check_batch(G, ss, hay, needles, rows=(16, 128, 128), window=DEFAULT, want=want)


LENGTHS = np.array([0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 9000])


def ragged(rng, key_type):
    """300 segments with haystack and needle lengths drawn independently from LENGTHS; then 5000 consecutive segments without
    needles (and with short haystacks) between two needles of one tile; needles in front of the first offset and behind the last."""
    hl, nl = rng.choice(LENGTHS, 300), rng.choice(LENGTHS, 300)
    hl[:10] = LENGTHS  # every length on either side at least once, and needles with an empty haystack
    nl[:10] = LENGTHS[::-1]
    nl[10], hl[10] = 65, 0
    nl[299] = 1
    hl, nl = np.concatenate([hl, rng.integers(0, 3, 5000), [70]]), np.concatenate([nl, np.zeros(5000, dtype=np.int64), [1]])
    ho, no = offsets_of(hl), offsets_of(nl, first=5)
    hay = sorted_rows(rng, ho, 700, key_type)
    needles = keys_of(rng.integers(0, 702, int(no[-1]) + 9), key_type)
    return hay, needles, ho, no


@pytest.mark.parametrize("key_type", ["uint32", "int64"])
def test_ragged_segments_from_both_offsets(G, key_type):
    rng = np.random.default_rng(300)
    hay, needles, ho, no = ragged(rng, key_type)
    ss = G.SortedSearch()
    want = check_batch(G, ss, hay, needles, ho, no, shifts=(0, 8, 12))
    check_batch(G, ss, hay, needles, ho, no, window=0, want=want, shifts=(8, 0, 4))
    check_batch(G, ss, hay, needles, ho, no, outputs="upper", window=64, want=want)
    assert (want[0][:5] == POISON32).all() and (want[1][-9:] == POISON32).all()  # uncovered in front and behind
    empty = np.flatnonzero((np.diff(ho.astype(np.int64)) == 0) & (np.diff(no.astype(np.int64)) > 0))
    assert empty.size >= 2
    for s in empty:  # needles with an empty haystack: all 0
        assert (want[0][no[s]:no[s + 1]] == 0).all() and (want[1][no[s]:no[s + 1]] == 0).all()
    # the run of 5000 segments without needles lies between the last two needles, inside one tile
    assert no[300] == no[5300] and no[5301] == no[300] + 1 and no[300] - no[299] == 1


@pytest.mark.parametrize("key_type", ["float32", "uint64"])
def test_equal_needle_rows_over_ragged_haystacks(G, key_type):
    """needle_offsets NULL: M samples for each of the ragged rows, the sampling case."""
    rng = np.random.default_rng(77)
    hl = rng.choice(LENGTHS, 120)
    hl[:10] = LENGTHS
    ho = offsets_of(hl)
    hay = sorted_rows(rng, ho, 700, key_type)
    ss = G.SortedSearch()
    for M in (1, 37, 2500):
        needles = keys_of(rng.integers(0, 702, 120 * M), key_type)
        want = check_batch(G, ss, hay, needles, ho, None, window=DEFAULT)
        check_batch(G, ss, hay, needles, ho, None, window=0, want=want, outputs="lower")


def test_one_segment_is_the_single_call(G):
    import torch

    rng = np.random.default_rng(1)
    hay = np.sort(rng.integers(0, 30000, 100003).astype(np.uint32))
    needles = rng.integers(0, 30010, 5000).astype(np.uint32)
    ss = G.SortedSearch()
    want = check_batch(G, ss, hay, needles, np.array([0, hay.size]), np.array([0, needles.size]))
    check_batch(G, ss, hay, needles, rows=(1, hay.size, needles.size), want=want)
    ha, na, lo, up = Array(hay), Array(needles), Array.poisoned(4 * needles.size), Array.poisoned(4 * needles.size)
    ss.run_ptr(ha.ptr, hay.size, na.ptr, needles.size, lo.ptr, up.ptr, "uint32", False, stream())
    torch.cuda.synchronize()
    assert (lo.result(np.uint32) == want[0]).all() and (up.result(np.uint32) == want[1]).all()


def float_specials(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    top = 8 * np.dtype(dtype).itemsize - 1
    quiet = (u(0x7FC) << u(top - 11)) if dtype == np.float32 else (u(0x7FF8) << u(top - 15))
    nans = np.array([quiet | u(1), quiet | u(0x12345), (u(1) << u(top)) | quiet | u(1), (u(1) << u(top)) | quiet | u(0x12345)], dtype=u).view(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    return np.concatenate([np.array([-0.0, 0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5, np.finfo(dtype).max, np.finfo(dtype).min], dtype=dtype), nans])


@pytest.mark.parametrize("key_type", ["float32", "float64", "int32", "int64", "uint32"])
def test_key_contents(G, key_type):
    """A row of one repeated key (lower 0, upper len); needles below and above every key; floats with both zeros, the infinities and
    NaNs of both signs in the sort's order; signed keys around 0."""
    dtype = np.dtype(key_type)
    rng = np.random.default_rng(9)
    if dtype.kind == "f":
        special = float_specials(dtype.type)
    elif dtype.kind == "i":
        info = np.iinfo(dtype)
        special = np.array([info.min, info.min + 1, -2, -1, 0, 1, 2, info.max - 1, info.max], dtype=dtype)
    else:
        special = np.array([0, 1, 2, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1], dtype=dtype)
    rows = []
    for s in range(6):  # every row: the special keys, some of them repeated, in the sort's order
        row = np.concatenate([special, special[rng.integers(0, special.size, 20 + s)]])
        rows.append(row[np.argsort(enc(row), kind="stable")])
    rows.append(np.full(333, special[4], dtype=dtype))  # one repeated key
    rows.append(special[:0])  # no key
    mid = special[np.argsort(enc(special))][1:-1]  # a row that lacks the smallest and the largest key: they lie below and above it
    rows.append(mid)
    ho = offsets_of([r.size for r in rows])
    hay = np.concatenate(rows)
    per = np.concatenate([special, special, special[::-1]])
    needles = np.concatenate([per] * len(rows))
    no = offsets_of([per.size] * len(rows))
    ss = G.SortedSearch()
    want = check_batch(G, ss, hay, needles, ho, no)
    check_batch(G, ss, hay, needles, ho, no, window=0, want=want)
    check_batch(G, ss, hay, needles, ho, None, want=want)
    one = slice(int(no[6]), int(no[7]))
    hit = enc(needles[one]) == enc(special[4:5])[0]
    assert (want[0][one][hit] == 0).all() and (want[1][one][hit] == 333).all() and hit.sum() == 3
    last = slice(int(no[8]), int(no[9]))
    assert want[1][last].min() == 0 and want[0][last].max() == mid.size  # below every key, above every key
    if dtype.kind == "f":
        first = slice(0, special.size)  # the first row holds -0.0 in front of +0.0, and the NaNs beyond the infinities
        neg0, pos0 = want[0][first][0], want[0][first][1]
        assert pos0 > neg0 and want[1][first][0] == pos0
        assert want[0][first][10] > want[0][first][2] and want[0][first][12] < want[0][first][3]  # +NaN above +inf, -NaN below -inf


def test_captured_from_the_first_call_and_replayed(G):
    """Both forms captured on one stream, each the FIRST call of a fresh object, and replayed on other contents of hay, needles and
    device offsets of the same totals.  The calls leave the device's free memory as they found it."""
    import torch

    P, n, m = 23, 200, 150
    S, hay_total, needle_total = 40, 6000, 5000
    ht = torch.empty(P * n, dtype=torch.int32, device="cuda")
    nt = torch.empty(P * m, dtype=torch.int32, device="cuda")
    h2 = torch.empty(hay_total, dtype=torch.int64, device="cuda")
    n2 = torch.empty(needle_total, dtype=torch.int64, device="cuda")
    hot, not_ = torch.empty(S + 1, dtype=torch.int32, device="cuda"), torch.empty(S + 1, dtype=torch.int32, device="cuda")
    outs = [torch.empty(c, dtype=torch.int32, device="cuda") for c in (P * m, P * m, needle_total, needle_total)]

    def content(seed):
        r = np.random.default_rng(seed)
        hay = sorted_rows(r, np.arange(P + 1) * n, 500, "uint32")
        needles = keys_of(r.integers(0, 502, P * m), "uint32")
        ho = offsets_of(r.multinomial(hay_total - 7, np.ones(S) / S) * (r.integers(0, 4, S) > 0))
        no = offsets_of(r.multinomial(needle_total - 11, np.ones(S) / S), first=3)
        hay2 = sorted_rows(r, np.concatenate([ho, [hay_total]]), 400, "uint64")
        needles2 = keys_of(r.integers(0, 402, needle_total), "uint64")
        return hay, needles, ho, no, hay2, needles2

    def fill(c):
        for t, a in zip((ht, nt, hot, not_, h2, n2), c):
            t.copy_(torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])))
        for o in outs:
            o.fill_(-1515870811)

    def verify(c):
        hay, needles, ho, no, hay2, needles2 = c
        w1 = expected(hay, np.arange(P + 1) * n, needles, np.arange(P + 1) * m)
        w2 = expected(hay2, ho, needles2, no)
        for o, w in zip(outs, w1 + w2):
            assert (o.cpu().numpy().view(np.uint32) == w).all()

    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    contents = [content(seed) for seed in (0, 1, 2)]
    a, b = G.SortedSearch(), G.SortedSearch()

    def call(s):
        a.run_batch_ptr(ht.data_ptr(), n, nt.data_ptr(), m, P, outs[0].data_ptr(), outs[1].data_ptr(), "uint32", s)
        b.run_batch_offsets_ptr(h2.data_ptr(), hay_total, hot.data_ptr(), n2.data_ptr(), needle_total, not_.data_ptr(), S, outs[2].data_ptr(),
                                outs[3].data_ptr(), "uint64", s)

    with torch.cuda.stream(side):
        fill(contents[0])
        side.synchronize()
        warm = G.SortedSearch()  # (another object loads the kernels)
        warm.run_batch_ptr(ht.data_ptr(), n, nt.data_ptr(), m, P, outs[0].data_ptr(), outs[1].data_ptr(), "uint32", side.cuda_stream)
        warm.run_batch_offsets_ptr(h2.data_ptr(), hay_total, hot.data_ptr(), n2.data_ptr(), needle_total, not_.data_ptr(), S, outs[2].data_ptr(),
                                   outs[3].data_ptr(), "uint64", side.cuda_stream)
        side.synchronize()
        verify(contents[0])
        fill(contents[0])
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)  # the first calls of a and b
        assert a.last() == (BATCH, 0, 1) and b.last() == (BATCH, 0, 1)
        for c in contents[::-1]:
            fill(c)
            graph.replay()
            side.synchronize()
            verify(c)
        assert torch.cuda.mem_get_info()[0] >= held - (64 << 20), "a call took device memory"  # (the graph itself takes a little)


def test_life_cycle_beside_the_single_calls(G):
    """index_ptr -> batched call -> run_ptr(reuse_index) still succeeds and is right; a batched call after a large single call; a
    small batched call after a large one, all on one object."""
    import torch

    rng = np.random.default_rng(4)
    ss = G.SortedSearch()
    hay = np.sort(rng.integers(0, 2**31, 1 << 20).astype(np.uint32))
    needles = rng.integers(0, 2**31, 40000).astype(np.uint32)
    ha, na = Array(hay), Array(needles)
    ss.index_ptr(ha.ptr, hay.size, "uint32", stream())
    assert ss.last()[0] == G.SearchPath_Indexed
    big_hay = sorted_rows(rng, np.arange(65) * 3000, 9000, "uint32")
    check_batch(G, ss, big_hay, keys_of(rng.integers(0, 9002, 64 * 2000), "uint32"), rows=(64, 3000, 2000))
    lo, up = Array.poisoned(4 * needles.size), Array.poisoned(4 * needles.size)
    ss.run_ptr(ha.ptr, hay.size, na.ptr, needles.size, lo.ptr, up.ptr, "uint32", True, stream())
    torch.cuda.synchronize()
    assert ss.last() == (G.SearchPath_Indexed, G.plan_sorted_search(hay.size, needles.size)[1], 1)
    assert (lo.result(np.uint32) == np.searchsorted(hay, needles, "left")).all()
    assert (up.result(np.uint32) == np.searchsorted(hay, needles, "right")).all()
    small = sorted_rows(rng, np.arange(4) * 10, 30, "uint64")
    check_batch(G, ss, small, keys_of(rng.integers(0, 32, 3 * 7), "uint64"), rows=(3, 10, 7))
    check_batch(G, ss, small[:0], small[:0], rows=(0, 10, 7))  # nothing to do
    assert ss.last() == (BATCH, 0, 0)


def test_nothing_to_do_accepts_null_arrays(G):
    ss = G.SortedSearch()
    for call in (lambda: ss.run_batch_ptr(None, 5, None, 7, 0, None, None, "uint32", stream()),
                 lambda: ss.run_batch_ptr(None, 5, None, 0, 9, None, None, "float64", stream()),
                 lambda: ss.run_batch_offsets_ptr(None, 0, None, None, 0, None, 0, None, None, "int32", stream()),
                 lambda: ss.run_batch_offsets_ptr(None, 100, None, None, 0, None, 10, None, None, "int64", stream()),
                 lambda: ss.run_batch_offsets_ptr(None, 100, None, None, 50, None, 0, None, None, "uint64", stream())):
        ss.index_ptr(None, 0, "uint32", stream())
        assert ss.last()[0] != BATCH
        call()
        assert ss.last() == (BATCH, 0, 0)


def test_every_refusal_names_its_argument_and_writes_nothing(G):
    import torch

    rng = np.random.default_rng(8)
    S, n, m = 6, 50, 40
    hay = sorted_rows(rng, np.arange(S + 1) * n, 90, "uint32")
    needles = keys_of(rng.integers(0, 92, S * m), "uint32")
    ha, na = Array(hay), Array(needles)
    hoa, noa = Array((np.arange(S + 1) * n).astype(np.uint32)), Array((np.arange(S + 1) * m).astype(np.uint32))
    lo, up = Array.poisoned(4 * S * m), Array.poisoned(4 * S * m)
    ss = G.SortedSearch()
    raw = G.lib()

    def part(hay_p=ha.ptr, hay_count=n, needles_p=na.ptr, needle_count=m, P=S, lower=lo.ptr, upper=up.ptr, key_type=0, search=ss._h):
        return raw.glu_sorted_search_run_batch_ptr(search, hay_p, hay_count, needles_p, needle_count, P, key_type, lower, upper, stream())

    def offs(hay_p=ha.ptr, hay_total=S * n, ho=hoa.ptr, needles_p=na.ptr, needle_total=S * m, no=noa.ptr, segments=S, lower=lo.ptr,
             upper=up.ptr, key_type=0, search=ss._h):
        return raw.glu_sorted_search_run_batch_offsets_ptr(search, hay_p, hay_total, ho, needles_p, needle_total, no, segments, key_type, lower,
                                                           upper, stream())

    cases = [
        (lambda: part(search=None), "search is NULL"),
        (lambda: offs(search=None), "search is NULL"),
        (lambda: part(hay_p=None), "Invalid hay buffer"),
        (lambda: offs(hay_p=None), "Invalid hay buffer"),
        (lambda: part(needles_p=None), "Invalid needles buffer"),
        (lambda: offs(needles_p=None), "Invalid needles buffer"),
        (lambda: offs(ho=None), "hay_offsets is NULL"),
        (lambda: part(lower=None, upper=None), "out_lower and out_upper are both NULL"),
        (lambda: offs(lower=None, upper=None), "out_lower and out_upper are both NULL"),
        (lambda: part(hay_p=ha.ptr + 2), "hay is not aligned to the key size"),
        (lambda: part(hay_p=ha.ptr + 4, key_type=3), "hay is not aligned to the key size"),
        (lambda: offs(needles_p=na.ptr + 1), "needles is not aligned to the key size"),
        (lambda: part(lower=lo.ptr + 2), "out_lower is not aligned to 4 bytes"),
        (lambda: offs(upper=up.ptr + 1), "out_upper is not aligned to 4 bytes"),
        (lambda: offs(ho=hoa.ptr + 2), "hay_offsets is not aligned to 4 bytes"),
        (lambda: offs(no=noa.ptr + 3), "needle_offsets is not aligned to 4 bytes"),
        (lambda: part(key_type=6), "Invalid key type: 6"),
        (lambda: offs(key_type=-1), "Invalid key type: -1"),
        (lambda: part(hay_count=2**29, P=8), "hay_count * num_partitions must stay below 2^32"),
        (lambda: part(needle_count=2**31, P=2), "needle_count * num_partitions must stay below 2^32"),
        (lambda: part(hay_count=0, needle_count=0, P=2**32), "hay_count * num_partitions must stay below 2^32"),
        (lambda: offs(segments=2**24 + 1), "num_segments 16777217 exceeds 2^24"),
        (lambda: offs(hay_total=2**32), "a batch must hold fewer than 2^32 elements"),
        (lambda: offs(needle_total=2**32), "a batch must hold fewer than 2^32 elements"),
        (lambda: offs(no=None, needle_total=S * m - 1), "needle_total must be a multiple of num_segments where needle_offsets is NULL"),
        (lambda: part(lower=ha.ptr + 8), "out_lower overlaps hay"),
        (lambda: part(upper=na.ptr), "out_upper overlaps needles"),
        (lambda: offs(lower=hoa.ptr), "out_lower overlaps hay_offsets"),
        (lambda: offs(upper=noa.ptr + 4), "out_upper overlaps needle_offsets"),
        (lambda: part(upper=lo.ptr + 4 * (S * m - 1)), "out_upper overlaps out_lower"),
    ]
    for call, message in cases:
        assert call() == G.GLU_ERROR_INVALID_ARGUMENT, message
        got = raw.glu_last_error().decode()
        assert message in got, (message, got)
    # the window: its own range, then the range of the call's key width
    for keys in (1, 15, 8193, 2**31):
        assert raw.glu_sorted_search_set_batch_window(ss._h, keys) == G.GLU_ERROR_INVALID_ARGUMENT
        assert "the batch window must be 0 or lie in [16, 8192] (got %d)" % keys in raw.glu_last_error().decode()
    assert raw.glu_sorted_search_set_batch_window(None, 0) == G.GLU_ERROR_INVALID_ARGUMENT and "search is NULL" in raw.glu_last_error().decode()
    ss.set_batch_window(8192)
    h8, n8 = Array(hay.astype(np.uint64)), Array(needles.astype(np.uint64))
    assert part(hay_p=h8.ptr, needles_p=n8.ptr, key_type=3) == G.GLU_ERROR_INVALID_ARGUMENT
    assert "the batch window must be 0 or lie in [16, 4096] for 8-byte keys (got 8192)" in raw.glu_last_error().decode()
    torch.cuda.synchronize()
    # a refused call writes nothing, anywhere
    for a in (ha, na, hoa, noa, lo, up, h8, n8):
        assert a.unchanged()
    # arrays that merely touch are fine, and the object still works
    ss.set_batch_window(DEFAULT)
    both = Array.poisoned(8 * S * m)
    assert part(lower=both.ptr, upper=both.ptr + 4 * S * m) == 0
    torch.cuda.synchronize()
    want = expected(hay, np.arange(S + 1) * n, needles, np.arange(S + 1) * m)
    assert (both.result(np.uint32) == np.concatenate(want)).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_sorted_search_batch_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout


def need(nbytes):
    """Skips unless `nbytes` and 4 GiB more (the chunked fills, the allocator's slack) are free."""
    import torch

    assert nbytes <= 40 * GIB, "no test may need more than 40 GiB"
    if torch.cuda.mem_get_info()[0] < nbytes + 4 * GIB:
        pytest.skip("needs %d GiB of free HBM" % -(-(nbytes + 4 * GIB) // GIB))


@pytest.mark.parametrize("window", [DEFAULT, 0])
def test_positions_past_2_31(G, window):
    """A device-filled uint32 haystack of 2^31 + 2^20 keys, hay[i] = i, in 3 segments; the last one begins past 2^31.  2^16 needles
    per segment.  Needle v in the segment [hb, he) has lower = clamp(v - hb, 0, he - hb) and upper = clamp(v + 1 - hb, 0, he - hb).
    The rows are far longer than any window: the probes go to global memory."""
    import torch

    total = (1 << 31) + (1 << 20)
    need(4 * total)
    ho = np.array([0, (1 << 20) + 5, (1 << 31) + 7, total], dtype=np.int64)
    hay = torch.empty(total, dtype=torch.int32, device="cuda")
    step = 1 << 27
    for a in range(0, total, step):
        b = min(total, a + step)
        hay[a:b] = torch.arange(a, b, dtype=torch.int64, device="cuda").to(torch.int32)  # (wraps into the bits of the uint32 i)
    M = 1 << 16
    rng = np.random.default_rng(31)
    rows = []
    for s in range(3):
        hb, he = int(ho[s]), int(ho[s + 1])
        v = rng.integers(max(hb - 1000, 0), min(he + 1000, 2**32), M)
        special = [0, 2**32 - 1, hb, max(hb - 1, 0), hb + 1, he - 1, he, min(he + 1, 2**32 - 1), 2**31 - 1, 2**31, 2**31 + 1]
        v[:len(special)] = special
        rows.append(v)
    v = np.concatenate(rows)
    needles = Array(v.astype(np.uint32))
    hoa = Array(ho.astype(np.uint32))
    lo, up = Array.poisoned(4 * 3 * M), Array.poisoned(4 * 3 * M)
    ss = G.SortedSearch()
    ss.set_batch_window(window)
    ss.run_batch_offsets_ptr(hay.data_ptr(), total, hoa.ptr, needles.ptr, 3 * M, None, 3, lo.ptr, up.ptr, "uint32", stream())
    torch.cuda.synchronize()
    assert ss.last() == (BATCH, 0, 1)
    hb, length = np.repeat(ho[:3], M), np.repeat(np.diff(ho), M)
    assert (lo.result(np.uint32) == np.clip(v - hb, 0, length)).all()
    assert (up.result(np.uint32) == np.clip(v + 1 - hb, 0, length)).all()
    assert int(hay[0]) == 0 and int(hay[total - 1]) & 0xFFFFFFFF == total - 1 and needles.unchanged() and hoa.unchanged()
    assert np.clip(v - hb, 0, length).max() > 2**30  # a local position of more than 30 bits
    del hay
    torch.cuda.empty_cache()
