"""GPU tests of key runs (glu_key_runs_run_ptr): the heads of the runs of equal keys as an offsets array for the batched calls, the
key at every head and the number of runs.  Expected values come from numpy: heads = flatnonzero(r_[True, (k[1:] ^ k[:-1]) & mask
!= 0]).  Every array the call writes sits inside an allocation with poison in front of it and behind it, and is itself filled with
poison first, so that an entry the call must not touch still holds it.  Sizes come from plan_key_runs."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8  # elements of poison in front of and behind an array, inside its allocation


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def poison_of(dtype):
    return np.array([0xA5A5A5A5A5A5A5A5 & ((1 << (8 * np.dtype(dtype).itemsize)) - 1)], dtype=np.uint64).astype(dtype)[0]


class Array:
    """`d` on the device, `shift` elements behind the start of an allocation that holds poison in front of and behind it."""

    def __init__(self, d, shift=0):
        import torch

        d = np.ascontiguousarray(d)
        self.dtype, self.n, self.front = d.dtype, d.size, GUARD + shift
        p = poison_of(d.dtype)
        self.host = np.concatenate([np.full(self.front, p, dtype=d.dtype), d, np.full(GUARD, p, dtype=d.dtype)])
        self.t = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()
        self.ptr = self.t.data_ptr() + self.front * d.dtype.itemsize

    @classmethod
    def poisoned(cls, n, dtype):
        return cls(np.full(n, poison_of(dtype), dtype=dtype))

    def result(self):
        """The array after the call; asserts that the poison around it is intact."""
        raw = self.t.cpu().numpy().view(self.dtype)
        assert (raw[:self.front] == self.host[:self.front]).all() and (raw[self.front + self.n:] == self.host[self.front + self.n:]).all(), \
            "the call wrote outside the array"
        return raw[self.front:self.front + self.n].copy()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def mask_of(key_bits, begin_bit, end_bit):
    return ((1 << (end_bit - begin_bit)) - 1) << begin_bit


def heads_of(keys, mask):
    if keys.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero(np.r_[True, ((keys[1:] ^ keys[:-1]) & keys.dtype.type(mask)) != 0])


def expected(keys, mask, max_runs):
    heads = heads_of(keys, mask)
    m = min(heads.size, max_runs)
    offsets = np.full(max_runs + 1, keys.size, dtype=np.uint32)
    offsets[:m] = heads[:m]
    unique = np.full(max_runs, poison_of(keys.dtype), dtype=keys.dtype)
    unique[:m] = keys[heads[:m]]
    return offsets, unique, heads.size


def check_case(G, runs, keys, max_runs, begin_bit=0, end_bit=None, shift=0, with_unique=True):
    """One call on `keys` (numpy, uint32 or uint64); every output compared with `==`, the poison checked, the keys unchanged.
    Returns the number of runs."""
    import torch

    key_bits = 8 * keys.dtype.itemsize
    end_bit = key_bits if end_bit is None else end_bit
    ka = Array(keys, shift)
    oa = Array.poisoned(max_runs + 1, np.uint32)
    ua = Array.poisoned(max_runs, keys.dtype)
    na = Array.poisoned(1, np.uint32)
    runs.run_ptr(ka.ptr if keys.size else None, keys.size, oa.ptr, max_runs, na.ptr, ua.ptr if with_unique else None, key_bits, begin_bit,
                 end_bit, stream())
    torch.cuda.synchronize()
    want_offsets, want_unique, want_runs = expected(keys, mask_of(key_bits, begin_bit, end_bit), max_runs)
    what = (keys.size, max_runs, key_bits, begin_bit, end_bit, shift)
    assert int(na.result()[0]) == want_runs, what
    got = oa.result()
    bad = np.flatnonzero(got != want_offsets)
    assert bad.size == 0, (what, int(bad[0]), int(got[bad[0]]), int(want_offsets[bad[0]]))
    got = ua.result()
    if not with_unique:
        want_unique = np.full(max_runs, poison_of(keys.dtype), dtype=keys.dtype)
    bad = np.flatnonzero(got != want_unique)
    assert bad.size == 0, (what, int(bad[0]), hex(int(got[bad[0]])), hex(int(want_unique[bad[0]])))
    assert (ka.result() == keys).all(), "the call wrote to its keys"
    return want_runs


def widen(k, dtype):
    """uint32 patterns as keys of `dtype`: 8-byte keys carry them across the boundary of their two words."""
    k = np.asarray(k, dtype=np.uint64)
    return k.astype(np.uint32) if np.dtype(dtype) == np.uint32 else (k << np.uint64(31)) | np.uint64(5)


def random_runs(rng, n, mean=3):
    """n keys in runs of random lengths (geometric, the given mean); neighbouring runs differ."""
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    lens = rng.geometric(1.0 / mean, int(1.5 * n / mean) + 64)
    while lens.sum() < n:
        lens = np.concatenate([lens, rng.geometric(1.0 / mean, lens.size)])
    m = int(np.searchsorted(np.cumsum(lens), n)) + 1
    values = np.cumsum(rng.integers(1, 1000, m))
    return np.repeat(values, lens[:m])[:n].astype(np.uint64)


PATTERNS = ["all_equal", "all_distinct", "random_runs", "heads_on_tile_starts", "runs_across_tile_boundaries", "heads_on_first_lanes"]


def pattern(name, rng, n, tile):
    i = np.arange(n, dtype=np.uint64)
    if name == "all_equal":
        return np.full(n, 7, dtype=np.uint64)
    if name == "all_distinct":
        return i * np.uint64(3) + np.uint64(1)
    if name == "random_runs":
        return random_runs(rng, n)
    if name == "heads_on_tile_starts":
        return i // np.uint64(tile)
    if name == "runs_across_tile_boundaries":  # keys[tile - 1] == keys[tile]: the runs change in the middle of every tile
        return (i + np.uint64(tile // 2)) // np.uint64(tile)
    # a tile is 4 waves x 4 packs per lane: lane 0 of a wave holds the keys at the multiples of tile / 16
    return i // np.uint64(tile // 16)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_boundaries(G, dtype, name):
    tile = G.plan_key_runs(1, 8 * np.dtype(dtype).itemsize)[0]
    rng = np.random.default_rng(PATTERNS.index(name))
    runs = G.KeyRuns()
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1):
        keys = widen(pattern(name, rng, n, tile), dtype)
        got = check_case(G, runs, keys, n)
        if name == "all_equal":
            assert got == min(n, 1)
        if name == "all_distinct":
            assert got == n
        if name == "runs_across_tile_boundaries" and n > tile:
            assert keys[tile - 1] == keys[tile]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_capacity(G, dtype):
    """max_runs below, at and above the number of runs: every one of the max_runs + 1 offsets, num_runs the true number, and the
    entries of unique_keys behind min(R, max_runs) still poison (expected() fills them with it)."""
    rng = np.random.default_rng(20)
    keys = widen(random_runs(rng, 3000), dtype)
    R = heads_of(keys, ~0 & ((1 << (8 * keys.dtype.itemsize)) - 1)).size
    assert 800 < R < 1300
    runs = G.KeyRuns()
    for max_runs in (0, 1, R - 1, R, R + 1, R + 4097):
        assert check_case(G, runs, keys, max_runs) == R
        assert expected(keys, (1 << (8 * keys.dtype.itemsize)) - 1, max_runs)[0][max_runs] == keys.size
    check_case(G, runs, keys, R + 3, with_unique=False)  # NULL unique_keys: skipped


@pytest.mark.parametrize("dtype,shift", [(np.uint32, 1), (np.uint32, 2), (np.uint32, 3), (np.uint64, 1)])
def test_misaligned_bases(G, dtype, shift):
    """Keys that start 1, 2, 3 elements behind a 16-byte boundary: the tiles are counted from that boundary, so the last tile's
    keys move too (tile + 5 keys: two tiles; 2 * tile - 1 keys: a tile more than the plan's when the base is not aligned)."""
    tile = G.plan_key_runs(1, 8 * np.dtype(dtype).itemsize)[0]
    rng = np.random.default_rng(30 + shift)
    runs = G.KeyRuns()
    for n in (tile + 5, 2 * tile - 1, 2 * tile):
        for name in ("random_runs", "all_distinct", "heads_on_tile_starts"):
            keys = widen(pattern(name, rng, n, tile), dtype)
            assert Array(keys[:1], shift).ptr % 16 == shift * keys.dtype.itemsize
            check_case(G, runs, keys, n, shift=shift)


def test_bit_ranges(G):
    """Keys that agree on the bits of the range inside a run and differ outside it: the heads follow the range alone, and
    unique_keys carries the whole key at every head."""
    rng = np.random.default_rng(40)
    tile = G.plan_key_runs(1, 32)[0]
    n = tile + 77
    group = random_runs(rng, n, mean=5)
    runs = G.KeyRuns()
    k32 = (((group & np.uint64(0xFFFF)) << np.uint64(8)) | rng.integers(0, 256, n).astype(np.uint64)
           | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(24))).astype(np.uint32)
    by_range = check_case(G, runs, k32, n, 8, 24)
    assert by_range == heads_of((group & np.uint64(0xFFFF)), 0xFFFF).size < n // 3
    assert check_case(G, runs, k32, n, 0, 32) > n * 0.9
    assert check_case(G, runs, k32, n, 0, 8) > n * 0.9
    for bit in (0, 13, 32):
        assert check_case(G, runs, k32, n, bit, bit) == 1
    k64 = (group << np.uint64(32)) | rng.integers(0, 2**32, n).astype(np.uint64)
    assert check_case(G, runs, k64, n, 32, 64) == heads_of(group, (1 << 32) - 1).size
    assert check_case(G, runs, k64, n, 0, 64) > n * 0.9
    assert check_case(G, runs, k64, n, 0, 32) > n * 0.9
    assert check_case(G, runs, k64, n, 31, 33) > 1
    for bit in (0, 32, 64):
        assert check_case(G, runs, k64, n, bit, bit) == 1
    assert check_case(G, runs, k64[:0], 4, 5, 5) == 0


@pytest.mark.parametrize("more_tiles", [0, 1])
def test_two_rounds_of_the_count_scan(G, more_tiles):
    """The smallest count whose tile counts take two rounds of their scan (and, second case, a tile and three keys more, so that
    the second round's first tile is full).  Heads are sparse: one per 1000 keys, plus one at the first and one at the last key
    of the second round's first tile."""
    import torch

    tile = G.plan_key_runs(1, 32)[0]
    lo, hi = 1, 1 << 31  # rounds(lo) < 2 <= rounds(hi)
    assert G.plan_key_runs(hi, 32)[2] >= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if G.plan_key_runs(mid, 32)[2] >= 2:
            hi = mid
        else:
            lo = mid
    assert G.plan_key_runs(hi, 32)[2] == 2 and G.plan_key_runs(hi - 1, 32)[2] == 1
    first = G.plan_key_runs(hi - 1, 32)[1] * tile  # the first key of the second round's first tile
    n = hi + more_tiles * (tile + 3)
    assert first < n < 1 << 26 and G.plan_key_runs(n, 32)[2] == 2
    flags = np.zeros(n, dtype=bool)
    flags[::1000] = True
    flags[first] = True
    flags[min(first + tile, n) - 1] = True
    keys = np.cumsum(flags, dtype=np.uint32) * np.uint32(2654435761)
    heads = np.flatnonzero(flags)
    max_runs = heads.size + 7
    kt = torch.from_numpy(keys.view(np.int32)).cuda()
    oa, ua, na = Array.poisoned(max_runs + 1, np.uint32), Array.poisoned(max_runs, np.uint32), Array.poisoned(1, np.uint32)
    G.KeyRuns().run_ptr(kt.data_ptr(), n, oa.ptr, max_runs, na.ptr, ua.ptr, stream=stream())
    torch.cuda.synchronize()
    assert int(na.result()[0]) == heads.size
    want = np.full(max_runs + 1, n, dtype=np.uint32)
    want[:heads.size] = heads
    got = oa.result()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    want = np.full(max_runs, poison_of(np.uint32), dtype=np.uint32)
    want[:heads.size] = keys[heads]
    assert (ua.result() == want).all()
    assert (kt.cpu().numpy().view(np.uint32) == keys).all()
    del kt
    torch.cuda.empty_cache()


def test_keys_are_only_read_and_outputs_may_not_overlap_them(G):
    import torch

    rng = np.random.default_rng(60)
    n = 5000
    keys = widen(random_runs(rng, n), np.uint32)
    runs = G.KeyRuns()
    check_case(G, runs, keys, n)  # (compares the keys after the call with the keys before it)
    kt = torch.from_numpy(keys.view(np.int32)).cuda()
    other = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    kp, op = kt.data_ptr(), other.data_ptr()
    inside, behind = kp + 4 * (n - 1), kp + 4 * n
    assert heads_of(keys[100:n - 100], 0xFFFFFFFF).size > 99
    bad = [
        (lambda: runs.run_ptr(kp, n, inside, 100, op, op + 16), "offsets array overlaps keys"),
        (lambda: runs.run_ptr(kp, n, kp - 4 * 100, 100, op, op + 16), "offsets array overlaps keys"),
        (lambda: runs.run_ptr(kp, n, op, 100, op + 1024, inside), "unique_keys overlaps keys"),
        (lambda: runs.run_ptr(kp, n, op, 100, inside, None), "num_runs overlaps keys"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (kt.cpu().numpy().view(np.uint32) == keys).all()
    # arrays that only touch the keys are fine: offsets that end where the keys begin, unique_keys that begin where they end
    part = keys[100:n - 100]
    runs.run_ptr(kp + 400, n - 200, kp, 99, op, behind - 400, stream=stream())
    torch.cuda.synchronize()
    got = kt.cpu().numpy().view(np.uint32)
    want_offsets, want_unique, _ = expected(part, 0xFFFFFFFF, 99)
    assert (got[100:n - 100] == part).all()
    assert (got[:100] == want_offsets).all()
    assert (got[n - 100:n - 1] == want_unique).all() and got[n - 1] == keys[n - 1]


def test_sort_then_by_key(G):
    """float32 keys from a small alphabet with both zeros, two NaN payloads and both infinities, uint32 values: sort_typed_ptr,
    then the runs, then Reduce.run_by_key_ptr (Sum, Max), BlellochScan.run_by_key_ptr and a batched sort by a second key inside
    every run -- against a numpy group-by on the BIT PATTERNS of the unsorted input and numpy's lexsort."""
    import torch

    rng = np.random.default_rng(70)
    alphabet = np.array([0x80000000, 0x00000000, 0x7FC00001, 0x7FC12345, 0x7F800000, 0xFF800000, 0x3FC00000, 0xC0100000, 0x40400000,
                         0x00000123, 0xFFC00001], dtype=np.uint32)  # -0, +0, two NaNs, +inf, -inf, 1.5, -2.25, 3, a denormal, a negative NaN
    n = 20011
    bits = alphabet[rng.integers(0, alphabet.size, n)]
    vals = rng.integers(0, 2**32, n, dtype=np.uint32)
    R, max_runs = alphabet.size, alphabet.size + 5
    kt = torch.from_numpy(bits.view(np.int32)).cuda()
    vt = torch.from_numpy(vals.view(np.int32)).cuda()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "float32", stream())
    torch.cuda.synchronize()
    sk, sv = kt.cpu().numpy().view(np.uint32), vt.cpu().numpy().view(np.uint32)
    assert (np.sort(sk) == np.sort(bits)).all()
    heads = heads_of(sk, 0xFFFFFFFF)
    assert heads.size == R, "equal bit patterns are not side by side after the sort, or different ones were merged"
    group_of_input = {int(b): np.flatnonzero(bits == b) for b in alphabet}

    runs = G.KeyRuns()
    for op, fold, identity in ((G.ReduceOperator_Sum, lambda v: int(v.sum(dtype=np.uint64)) & 0xFFFFFFFF, 0),
                               (G.ReduceOperator_Max, lambda v: int(v.max()), 0)):
        oa, ua, na = Array.poisoned(max_runs + 1, np.uint32), Array.poisoned(max_runs, np.uint32), Array.poisoned(1, np.uint32)
        out = Array.poisoned(max_runs, np.uint32)
        G.Reduce(G.DataType_Uint, op).run_by_key_ptr(runs, kt.data_ptr(), vt.data_ptr(), out.ptr, n, oa.ptr, max_runs, na.ptr, ua.ptr,
                                                     stream=stream())
        torch.cuda.synchronize()
        assert int(na.result()[0]) == R
        unique, got = ua.result(), out.result()
        assert (unique[:R] == sk[heads]).all() and (unique[R:] == poison_of(np.uint32)).all()
        assert sorted(unique[:R].tolist()) == sorted(alphabet.tolist())  # (-0.0 and +0.0, the NaN payloads: all apart)
        for r in range(R):
            assert int(got[r]) == fold(vals[group_of_input[int(unique[r])]]), (op, r, hex(int(unique[r])))
        assert (got[R:] == identity).all()
        assert (oa.result() == expected(sk, 0xFFFFFFFF, max_runs)[0]).all()
    offsets = oa.result()

    # scan by key, on a copy of the sorted values
    st = vt.clone()
    oa2, na2 = Array.poisoned(max_runs + 1, np.uint32), Array.poisoned(1, np.uint32)
    G.BlellochScan(G.DataType_Uint).run_by_key_ptr(runs, kt.data_ptr(), st.data_ptr(), n, oa2.ptr, max_runs, na2.ptr, stream=stream())
    torch.cuda.synchronize()
    cum = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sv, dtype=np.uint64)])
    lens = np.diff(np.r_[heads, n])
    want = ((cum[:-1] - np.repeat(cum[heads], lens)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert (st.cpu().numpy().view(np.uint32) == want).all()
    assert (oa2.result() == offsets).all() and int(na2.result()[0]) == R

    # a second key inside every run: the batched sort over the same offsets, against lexsort (both stable)
    second = rng.integers(0, 50, n, dtype=np.uint32)
    payload = np.arange(n, dtype=np.uint32)
    st2 = torch.from_numpy(second.view(np.int32)).cuda()
    pt = torch.from_numpy(payload.view(np.int32)).cuda()
    G.RadixSort().sort_batch_offsets_ptr(st2.data_ptr(), pt.data_ptr(), n, oa2.ptr, max_runs, "uint32", stream())
    torch.cuda.synchronize()
    order = np.lexsort((second, np.repeat(np.arange(R), lens)))
    assert (st2.cpu().numpy().view(np.uint32) == second[order]).all()
    assert (pt.cpu().numpy().view(np.uint32) == order).all()
    assert (kt.cpu().numpy().view(np.uint32) == sk).all()


def test_by_key_float_sums_that_round(G):
    """Reduce by key over float32 values whose sums round: sorted uint32 keys with three runs of 3, 5 and 9 chunks of the batched
    reduce among a few hundred short ones, more than 256 runs apart.  The long runs' chunk slots are handed out in arrival
    order, and with odd chunk counts at least one run of partials starts at an odd slot.  Two calls give the same bits, and
    every long run's sum has the bits of the batched reduce of that slice alone, on the same array."""
    import torch

    chunk = 1  # float32 elements of the longest workgroup segment = of a chunk of a long one
    while G.plan_reduce_batch(2 * chunk, 4)[0] < 3:
        chunk *= 2
    assert G.plan_reduce_batch(chunk, 4) == (2, 1) and G.plan_reduce_batch(chunk + 1, 4) == (3, 2)
    rng = np.random.default_rng(71)
    lens = rng.integers(1, 40, 700)
    long_at = {5: 3, 330: 5, 650: 9}  # run: chunks
    for r, chunks in long_at.items():
        lens[r] = chunks * chunk - 7
        assert G.plan_reduce_batch(int(lens[r]), 4) == (3, chunks)
    heads = np.concatenate([[0], np.cumsum(lens)])
    n, R = int(heads[-1]), lens.size
    max_runs = R + 9
    keys = np.repeat(np.cumsum(rng.integers(1, 1000, R)).astype(np.uint32), lens)
    vals = rng.standard_normal(n).astype(np.float32)
    ka, va = Array(keys), Array(vals)
    runs, red = G.KeyRuns(), G.Reduce(G.DataType_Float, G.ReduceOperator_Sum)
    results = []
    for _ in range(2):
        oa, na, out = Array.poisoned(max_runs + 1, np.uint32), Array.poisoned(1, np.uint32), Array.poisoned(max_runs, np.float32)
        red.run_by_key_ptr(runs, ka.ptr, va.ptr, out.ptr, n, oa.ptr, max_runs, na.ptr, stream=stream())
        torch.cuda.synchronize()
        assert int(na.result()[0]) == R and (oa.result() == expected(keys, 0xFFFFFFFF, max_runs)[0]).all()
        assert red.read_batch()["long"] == 3
        results.append(out.result())
    assert (va.result().view(np.uint32) == vals.view(np.uint32)).all() and (ka.result() == keys).all()
    assert (results[0].view(np.uint8) == results[1].view(np.uint8)).all(), "the same call gave different bits"
    got = results[0]
    assert (got[R:] == 0).all()
    sums = np.add.reduceat(vals.astype(np.float64), heads[:-1])
    scale = np.add.reduceat(np.abs(vals).astype(np.float64), heads[:-1])
    assert (np.abs(got[:R] - sums) <= lens * float(np.finfo(np.float32).eps) * scale).all()  # (n * eps * sum|x|, as in the batched reduce's tests)
    for r, chunks in long_at.items():
        one, alone = Array(np.asarray([heads[r], heads[r + 1]], dtype=np.uint32)), Array.poisoned(1, np.float32)
        red.run_batch_offsets_ptr(va.ptr, alone.ptr, n, one.ptr, 1, stream())
        torch.cuda.synchronize()
        assert red.read_batch() == {"wave": 0, "block": 0, "long": 1}
        a, b = alone.result(), got[r:r + 1]
        print("run %d (%d chunks): by key %r, alone %r" % (r, chunks, float(b[0]), float(a[0])))
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), (r, chunks, float(b[0]), float(a[0]))


def test_argument_checks(G):
    import torch

    runs = G.KeyRuns()
    kt = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ot = torch.zeros(4096, dtype=torch.int32, device="cuda")
    kp, op = kt.data_ptr(), ot.data_ptr()
    up, np_ = op + 2048, op + 4096
    L, vp = G.lib(), ctypes.c_void_p
    bad = [
        (lambda: G.check(L.glu_key_runs_run_ptr(None, vp(kp), 64, 32, 0, 32, vp(up), vp(op), 4, vp(np_), None)), "runs is NULL"),
        (lambda: G.check(L.glu_key_runs_prepare(None, 64, 32)), "runs is NULL"),
        (lambda: G.check(L.glu_key_runs_create(None)), "out is NULL"),
        (lambda: runs.run_ptr(None, 64, op, 4, np_, up), "Invalid key buffer"),
        (lambda: runs.run_ptr(kp, 64, None, 4, np_, up), "Invalid offsets array"),
        (lambda: runs.run_ptr(kp, 64, op, 4, None, up), "Invalid num_runs pointer"),
        (lambda: runs.run_ptr(kp + 2, 64, op, 4, np_, up), "keys is not aligned"),
        (lambda: runs.run_ptr(kp + 4, 64, op, 4, np_, up, key_bits=64), "keys is not aligned"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up + 4, key_bits=64), "unique_keys is not aligned"),
        (lambda: runs.run_ptr(kp, 64, op + 2, 4, np_, up), "offsets array is not aligned"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_ + 1, up), "num_runs is not aligned"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up, key_bits=16), "key_bits"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up, key_bits=48), "key_bits"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up, begin_bit=9, end_bit=8), "Invalid bit range"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up, begin_bit=0, end_bit=33), "Invalid bit range"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, up, key_bits=64, begin_bit=0, end_bit=65), "Invalid bit range"),
        (lambda: runs.run_ptr(kp, 1 << 32, op, 4, np_, up), "fewer than 2^32"),
        (lambda: runs.run_ptr(kp, 64, op, 1 << 32, np_, up), "below 2^32"),
        (lambda: runs.prepare(1 << 32), "fewer than 2^32"),
        (lambda: runs.prepare(64, 12), "key_bits"),
        (lambda: runs.run_ptr(kp, 64, kp + 128, 4, np_, up), "offsets array overlaps keys"),
        (lambda: runs.run_ptr(kp, 64, op, 4, np_, kp), "unique_keys overlaps keys"),
        (lambda: runs.run_ptr(kp, 64, op, 4, kp + 252, up), "num_runs overlaps keys"),
        (lambda: G.plan_key_runs(8, 12), "key_bits"),
        (lambda: G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum).run_by_key_ptr(runs, kp, kp, op, 64, op + 8192, (1 << 24) + 1, np_), "2^24"),
        (lambda: G.BlellochScan(G.DataType_Uint).run_by_key_ptr(runs, kp, up, 64, op, (1 << 24) + 1, np_), "2^24"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (ot.cpu().numpy() == 0).all(), "a refused call wrote something"
    ot.fill_(-1)
    runs.run_ptr(None, 0, op, 4, np_, up)  # no keys: NULL keys are fine, every offset 0, no runs
    torch.cuda.synchronize()
    got = ot.cpu().numpy()
    assert (got[:5] == 0).all() and got[1024] == 0
    got[:5] = got[1024] = -1
    assert (got == -1).all()


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed on
    three different key contents with different numbers of runs (one of them above max_runs): the launch sequence does not depend
    on the data."""
    import torch

    tile = G.plan_key_runs(1, 32)[0]
    n, max_runs = 37 * tile + 11, 40000
    rng = np.random.default_rng(90)
    runs = G.KeyRuns()
    kt = torch.empty(n, dtype=torch.int32, device="cuda")
    ot = torch.empty(max_runs + 1, dtype=torch.int32, device="cuda")
    ut = torch.empty(max_runs, dtype=torch.int32, device="cuda")
    nt = torch.empty(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(keys):
        kt.copy_(torch.from_numpy(keys.view(np.int32)))
        ot.fill_(-1515870811)
        ut.fill_(-1515870811)
        nt.fill_(-1515870811)

    def verify(keys):
        want_offsets, want_unique, want_runs = expected(keys, 0xFFFFFFFF, max_runs)
        assert int(nt.cpu().numpy().view(np.uint32)[0]) == want_runs
        assert (ot.cpu().numpy().view(np.uint32) == want_offsets).all()
        assert (ut.cpu().numpy().view(np.uint32) == want_unique).all()
        return want_runs

    def call(s):
        runs.run_ptr(kt.data_ptr(), n, ot.data_ptr(), max_runs, nt.data_ptr(), ut.data_ptr(), stream=s)

    with torch.cuda.stream(side):
        keys = widen(random_runs(rng, n, mean=7), np.uint32)
        fill(keys)
        side.synchronize()
        runs.prepare(n)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(keys)
        fill(keys)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(keys)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        seen = []
        for mean in (2, 40, 5000):
            keys = widen(random_runs(rng, n, mean=mean), np.uint32)
            fill(keys)
            graph.replay()
            side.synchronize()
            seen.append(verify(keys))
        assert seen[0] > max_runs > seen[1] > seen[2] > 0, seen


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_key_runs_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
