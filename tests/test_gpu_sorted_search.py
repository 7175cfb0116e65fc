"""GPU tests of sorted search (glu_sorted_search_run_ptr): the lower and the upper bound of many needles in a sorted haystack, on
both paths.  Expected values are always numpy.searchsorted(enc(hay), enc(needles), side) on the keys as the sort encodes them
(unsigned, in the sort's order), compared with `==`.  Every array the call writes sits inside an allocation with poison in front of
it and behind it, and is itself filled with poison first; the inputs are checked unchanged.  The scheme is that of
test_gpu_select.py."""
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
AUTO, DIRECT, INDEXED = 0, 1, 2
KEYS = {"uint32": np.uint32, "int32": np.uint32, "float32": np.uint32, "uint64": np.uint64, "int64": np.uint64, "float64": np.uint64}


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


def bounds(hay, needles):
    """numpy's answer on the encoded keys; `hay` sorted in the sort's order."""
    eh, en = enc(hay), enc(needles)
    assert (eh[1:] >= eh[:-1]).all(), "the test's haystack is not sorted"
    return np.searchsorted(eh, en, "left").astype(np.uint32), np.searchsorted(eh, en, "right").astype(np.uint32)


def expected_last(G, path, hay_count, needle_count, key_type, top_entries=0, reuse=False):
    """(path, levels, kernels) as the header states them."""
    auto, levels, _, _ = G.plan_sorted_search(hay_count, needle_count, key_type, top_entries)
    taken = DIRECT if levels == 0 or path == DIRECT else INDEXED if path == INDEXED or reuse else auto
    search = 1 if needle_count else 0
    if taken == DIRECT:
        return (DIRECT, 0, search)
    return (INDEXED, levels, search + (0 if reuse else 1))


def check_case(G, ss, hay, needles, outputs="both", path=None, top_entries=0, hay_shift=0, needles_shift=0, out_shift=0, reuse=False,
               hay_array=None, want=None):
    """One call.  `hay` sorted in the sort's order, of one of the six key types; `needles` of the same type.  Every output compared
    with `==`, the poison checked, the inputs unchanged, last() as expected.  Returns (lower, upper) as numpy gives them."""
    import torch

    key_type = str(hay.dtype)
    assert needles.dtype == hay.dtype
    ha = hay_array or Array(hay, hay_shift)
    na = Array(needles, needles_shift)
    lo = Array.poisoned(4 * needles.size, out_shift)
    up = Array.poisoned(4 * needles.size, out_shift)
    if path is not None:
        ss.set_option("PATH", path)
    ss.run_ptr(ha.ptr if hay.size else None, hay.size, na.ptr if needles.size else None, needles.size,
               lo.ptr if outputs in ("both", "lower") else None, up.ptr if outputs in ("both", "upper") else None, key_type, reuse, stream())
    torch.cuda.synchronize()
    what = (key_type, hay.size, needles.size, outputs, path, top_entries, hay_shift, needles_shift, out_shift, reuse)
    if path is not None:
        assert ss.last() == expected_last(G, path, hay.size, needles.size, key_type, top_entries, reuse), (what, ss.last())
    want = want or bounds(hay, needles)
    for name, arr, w in (("lower", lo, want[0]), ("upper", up, want[1])):
        got = arr.result(np.uint32)
        if outputs not in ("both", name):
            w = np.full(needles.size, POISON32, dtype=np.uint32)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, (what, name, int(bad[0]), int(got[bad[0]]), int(w[bad[0]]))
    u = KEYS[key_type]
    assert (ha.result(u) == hay.view(u)).all(), "the call wrote to its haystack"
    assert (na.result(u) == needles.view(u)).all(), "the call wrote to its needles"
    return want


def sorted_hay(rng, n, dtype):
    """n sorted keys with duplicates (draws over a range three times narrower than n), three apart so that the keys between two
    of them are in no haystack; 8-byte keys use their high word."""
    draws = np.sort(rng.integers(0, n // 3 + 1, n)).astype(np.uint64)
    if np.dtype(dtype).itemsize == 8:
        return (draws * np.uint64(3 * 0x100000001) + np.uint64(1 << 40)).astype(dtype)
    return (draws * np.uint64(3) + np.uint64(1000)).astype(dtype)


def needles_for(rng, hay, count, fanout):
    """`count` random draws over the haystack's range (a third of them keys of the haystack), every key at a node edge with the
    keys just below and above it, and the type's smallest and largest key."""
    dtype = hay.dtype
    info = np.iinfo(dtype)
    parts = [np.array([info.min, info.max], dtype=dtype)]
    if hay.size:
        lo, hi = int(hay[0]), int(hay[-1])
        parts.append(rng.integers(max(lo - 5, info.min), min(hi + 5, info.max), count, dtype=dtype, endpoint=True))
        parts.append(hay[rng.integers(0, hay.size, count // 3)])
        i = np.arange(hay.size)
        edge = hay[(i % fanout == 0) | (i % fanout == 1) | (i % fanout == fanout - 1) | (i == hay.size - 1)]
        parts += [edge, edge - dtype.type(1), edge + dtype.type(1)]  # (the keys lie far from the ends of the type: no wrap)
    else:
        parts.append(rng.integers(0, 1000, count).astype(dtype))
    return rng.permutation(np.concatenate(parts))


@pytest.mark.parametrize("path", [DIRECT, INDEXED])
@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_level_boundaries(G, key_type, path):
    """TOP_ENTRIES = F, so that haystacks of F, F^2 and F^3 keys are where the index gains a level: every count around them, both
    paths, the three output forms."""
    dtype = np.dtype(key_type)
    F = 128 // dtype.itemsize
    rng = np.random.default_rng(F + path)
    ss = G.SortedSearch()
    ss.set_option("TOP_ENTRIES", F)
    seen = set()
    for n in (0, 1, F - 1, F, F + 1, F * F - 1, F * F, F * F + 1, F ** 3 - 1, F ** 3, F ** 3 + 1, F ** 3 + F * F + F + 7):
        hay = sorted_hay(rng, n, dtype)
        needles = needles_for(rng, hay, 3000, F)
        want = None
        for outputs in ("lower", "upper", "both"):
            want = check_case(G, ss, hay, needles, outputs, path, F, want=want)
        if n >= F * F:  # present and absent needles, and keys with copies
            assert (want[1] > want[0]).sum() > needles.size // 5 and (want[1] == want[0]).sum() > needles.size // 4
            assert (want[1] - want[0]).max() > 1
        seen.add(ss.last())
    if path == INDEXED:
        assert {levels for _, levels, _ in seen} == {0, 1, 2, 3}
        assert (DIRECT, 0, 1) in seen and (INDEXED, 3, 2) in seen  # (F keys or fewer have no index: the call is DIRECT)
    else:
        assert seen == {(DIRECT, 0, 1)}


@pytest.mark.parametrize("more", [31, 33])
def test_one_real_top_level(G, more):
    """The default TOP_ENTRIES (what LDS holds) and 2^16 needles.  8192 * 32 + 31 keys: one level of 8192 entries, the LDS table
    full.  8192 * 32 + 33 keys: 8193 entries do not fit any more, so a second level of 256 entries is the one in LDS."""
    n = 8192 * 32 + more
    rng = np.random.default_rng(more)
    hay = sorted_hay(rng, n, np.uint32)
    needles = needles_for(rng, hay, 1 << 16, 32)[:1 << 16]
    ss = G.SortedSearch()
    assert G.plan_sorted_search(n, needles.size)[:2] == (INDEXED, 1 if more == 31 else 2)
    want = check_case(G, ss, hay, needles, "both", AUTO)
    assert ss.last() == (INDEXED, 1 if more == 31 else 2, 2)
    check_case(G, ss, hay, needles, "both", DIRECT, want=want)


def float_specials(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    top = 8 * np.dtype(dtype).itemsize - 1
    quiet = (u(0x7FC) << u(top - 11)) if dtype == np.float32 else (u(0x7FF8) << u(top - 15))
    nans = np.array([quiet | u(1), quiet | u(0x12345), (u(1) << u(top)) | quiet | u(1), (u(1) << u(top)) | quiet | u(0x12345)], dtype=u).view(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    return np.concatenate([np.array([-0.0, 0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.finfo(dtype).max, np.finfo(dtype).min], dtype=dtype), nans])


@pytest.mark.parametrize("key_type", sorted(KEYS))
def test_six_key_types(G, key_type):
    """50 021 keys sorted by the library's own typed sort, then searched on the same stream: the search's order is the sort's.
    Floats hold both zeros, both infinities, denormals and NaNs of both signs with two payloads; signed types straddle zero."""
    import torch

    dtype = np.dtype(key_type)
    n = 50021
    rng = np.random.default_rng(len(key_type) + dtype.itemsize)
    if dtype.kind == "f":
        special = float_specials(dtype.type)
        hay = (rng.integers(-3000, 3000, n) / 16.0).astype(dtype)
        hay[rng.choice(n, 10 * special.size, replace=False)] = np.tile(special, 10)
        needles = np.concatenate([special, (rng.integers(-3100, 3100, 4000) / 16.0 + 1.0 / 64).astype(dtype), hay[rng.integers(0, n, 4000)]])
        assert np.isnan(hay).sum() == 40 and np.isnan(needles).sum() >= 4
    elif dtype.kind == "i":
        hay = rng.integers(-20000, 20000, n).astype(dtype) * dtype.type(3 if dtype.itemsize == 4 else 3 * 0x100000001)
        info = np.iinfo(dtype)
        needles = np.concatenate([np.array([info.min, -1, 0, 1, info.max], dtype=dtype), hay[rng.integers(0, n, 4000)] + dtype.type(1),
                                  hay[rng.integers(0, n, 4000)]])
        assert (hay < 0).sum() > n // 3 and (hay > 0).sum() > n // 3
    else:
        hay = rng.integers(0, 2 ** (8 * dtype.itemsize), n, dtype=dtype)
        hay[:n // 2] = hay[n // 2:2 * (n // 2)]  # (duplicates)
        needles = np.concatenate([np.array([0, np.iinfo(dtype).max], dtype=dtype), rng.integers(0, 2 ** (8 * dtype.itemsize), 4000, dtype=dtype),
                                  hay[rng.integers(0, n, 4000)]])
    needles = rng.permutation(needles)
    u = KEYS[key_type]
    ha = Array(hay)
    G.RadixSort().sort_typed_ptr(ha.ptr, None, n, key_type, stream())
    ss = G.SortedSearch()
    na, lo, up = Array(needles), Array.poisoned(4 * needles.size), Array.poisoned(4 * needles.size)
    ss.run_ptr(ha.ptr, n, na.ptr, needles.size, lo.ptr, up.ptr, key_type, stream=stream())  # (AUTO, no host read since the sort)
    torch.cuda.synchronize()
    assert ss.last() == (INDEXED, 1, 2)
    in_order = ha.result(u).view(dtype)
    assert (enc(in_order) == np.sort(enc(hay))).all(), "the typed sort's order is not the order of the encoded keys"
    want = bounds(in_order, needles)
    assert (lo.result(np.uint32) == want[0]).all() and (up.result(np.uint32) == want[1]).all()
    assert (want[1] > want[0]).sum() >= 4000 and (want[1] == want[0]).sum() >= 1000
    if dtype.kind == "f":  # -0.0 lies in front of +0.0, and a NaN is found as the key it is
        j = {name: int(np.flatnonzero(needles.view(u) == np.array([v], dtype=dtype).view(u)[0])[0]) for name, v in (("-0", -0.0), ("+0", 0.0))}
        assert want[1][j["-0"]] == want[0][j["+0"]] and want[1][j["-0"]] - want[0][j["-0"]] >= 10
        nan = np.flatnonzero(np.isnan(needles))
        assert (want[1][nan] - want[0][nan] >= 10).sum() >= 4
    sorted_array = Array(in_order)
    check_case(G, ss, in_order, needles, "both", DIRECT, hay_array=sorted_array, want=want)
    check_case(G, ss, in_order, needles, "both", INDEXED, hay_array=sorted_array, want=want)


@pytest.mark.parametrize("path", [DIRECT, INDEXED])
@pytest.mark.parametrize("key_type", ["int32", "float64"])
def test_degenerate_data(G, key_type, path):
    dtype = np.dtype(key_type)
    F = 128 // dtype.itemsize
    ss = G.SortedSearch()
    ss.set_option("TOP_ENTRIES", F)
    rng = np.random.default_rng(5)
    n = F * F + 3
    equal = np.full(n, 7, dtype=dtype)
    below, same, above = np.full(500, -9, dtype=dtype), np.full(500, 7, dtype=dtype), np.full(500, 8, dtype=dtype)
    lower, upper = check_case(G, ss, equal, np.concatenate([below, same, above]), "both", path, F)  # all keys equal
    assert (lower[:500] == 0).all() and (upper[:500] == 0).all() and (lower[500:1000] == 0).all() and (upper[500:1000] == n).all()
    assert (lower[1000:] == n).all() and (upper[1000:] == n).all()
    hay = np.sort(rng.integers(100, 200, n)).astype(dtype)
    for needles, where in ((np.full(700, 99, dtype=dtype), 0), (np.full(700, 200, dtype=dtype), n)):  # all needles below, all above
        lower, upper = check_case(G, ss, hay, needles, "both", path, F)
        assert (lower == where).all() and (upper == where).all()
    lower, upper = check_case(G, ss, hay, hay.copy(), "both", path, F)  # every needle a key
    assert (upper > lower).all()
    one = np.array([5], dtype=dtype)
    lower, upper = check_case(G, ss, one, np.array([4, 5, 6, 5], dtype=dtype), "both", path, F)  # a one-element haystack
    assert lower.tolist() == [0, 0, 1, 0] and upper.tolist() == [0, 1, 1, 1]
    lower, upper = check_case(G, ss, one[:0], np.array([4, 5, 6], dtype=dtype), "both", path, F)  # no haystack: NULL hay, zeros
    assert not lower.any() and not upper.any()


@pytest.mark.parametrize("path", [DIRECT, INDEXED])
@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_needle_tiles(G, key_type, path):
    """Needle counts around the wave and the tile, and the four arrays one element behind a 16-byte boundary, in turn and together
    (the needles' tiles are counted from the boundary: a shifted array can take a tile more)."""
    dtype = np.dtype(key_type)
    F, kb = 128 // dtype.itemsize, dtype.itemsize
    tile = G.SortedSearch.needle_tile(key_type)
    rng = np.random.default_rng(tile + path)
    ss = G.SortedSearch()
    ss.set_option("TOP_ENTRIES", F)
    hay = sorted_hay(rng, 5000, dtype)
    pool = needles_for(rng, hay, 40 * tile, F)
    assert Array(hay, kb).ptr % 16 == kb and Array.poisoned(64, 4).ptr % 16 == 4
    for count in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 37 * tile + 11):
        needles = pool[:count]
        want = check_case(G, ss, hay, needles, "both", path, F)
        for shifts in ((0, kb, 0), (kb, 0, 0), (0, 0, 4), (kb, kb, 4)):
            if count in (0, 65, tile, 37 * tile + 11):
                check_case(G, ss, hay, needles, "both", path, F, *shifts, want=want)
    assert ss.last() == expected_last(G, path, hay.size, 37 * tile + 11, key_type, F)
    check_case(G, ss, hay, pool[:tile], "upper", path, F, kb, kb, 4)
    check_case(G, ss, hay, pool[:tile], "lower", path, F, kb, kb, 4)


def test_reuse(G):
    """index_ptr once, then searches that enqueue one kernel each, a single needle among them; a call whose hay_count, key type or
    TOP_ENTRIES is not the index's is GLU_ERROR_INVALID_STATE, and so is reuse before any index."""
    rng = np.random.default_rng(8)
    n = 40000
    hay = sorted_hay(rng, n, np.uint32)
    ha = Array(hay)
    ss = G.SortedSearch()
    ss.set_option("TOP_ENTRIES", 32)
    na, lo = Array(hay[:64]), Array.poisoned(256)
    levels = G.plan_sorted_search(n, 1, "uint32", 32)[1]
    assert levels == 3 == G.plan_sorted_search(n + 5, 1, "uint32", 32)[1]

    def refused(call):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_STATE, e.value.message
        assert "reuse_index" in e.value.message
        return e.value.message

    assert "no index" in refused(lambda: ss.run_ptr(ha.ptr, n, na.ptr, 64, lo.ptr, None, "uint32", True, stream()))
    ss.index_ptr(ha.ptr, n, "uint32", stream())
    assert ss.last() == (INDEXED, levels, 1)
    for count in (3000, 1, 777):
        needles = needles_for(rng, hay, 3000, 32)[:count]
        check_case(G, ss, hay, needles, "both", None, 32, reuse=True, hay_array=ha)
        assert ss.last() == (INDEXED, levels, 1)
    refused(lambda: ss.run_ptr(ha.ptr, n - 1, na.ptr, 64, lo.ptr, None, "uint32", True, stream()))
    refused(lambda: ss.run_ptr(ha.ptr, n, na.ptr, 64, lo.ptr, None, "int32", True, stream()))
    refused(lambda: ss.run_ptr(ha.ptr + 4, n, na.ptr, 64, lo.ptr, None, "uint32", True, stream()))
    ss.set_option("TOP_ENTRIES", 64)
    refused(lambda: ss.run_ptr(ha.ptr, n, na.ptr, 64, lo.ptr, None, "uint32", True, stream()))
    ss.set_option("TOP_ENTRIES", 32)
    check_case(G, ss, hay, hay[:64].copy(), "lower", None, 32, reuse=True, hay_array=ha)  # (the index is still the haystack's)
    assert (lo.result(np.uint32) == POISON32).all(), "a refused call wrote something"
    # a call on the INDEXED path without reuse builds the index anew and remembers it
    other = sorted_hay(rng, n + 5, np.uint32)
    oa = Array(other)
    needles = needles_for(rng, other, 500, 32)
    want = check_case(G, ss, other, needles, "both", INDEXED, 32, hay_array=oa)
    assert ss.last() == (INDEXED, levels, 2)
    check_case(G, ss, other, needles, "both", INDEXED, 32, reuse=True, hay_array=oa, want=want)
    assert ss.last() == (INDEXED, levels, 1)
    refused(lambda: ss.run_ptr(ha.ptr, n, na.ptr, 64, lo.ptr, None, "uint32", True, stream()))


def test_argument_checks_and_overlaps(G):
    """One call per case the host can check, each with its own message; a witness buffer (every output lies in it) shows that the
    refused calls wrote nothing.  Outputs that only touch the inputs are accepted and correct."""
    import torch

    ss = G.SortedSearch()
    n = 4096
    hay = np.arange(n, dtype=np.uint32) * np.uint32(2)
    needles = np.random.default_rng(60).integers(0, 2 * n + 10, n, dtype=np.uint32)
    ht = torch.from_numpy(hay.view(np.int32).copy()).cuda()
    nt = torch.from_numpy(needles.view(np.int32).copy()).cuda()
    wt = torch.zeros(4 * n, dtype=torch.int32, device="cuda")  # the witness: out_lower, out_upper
    hp, np_, wp = ht.data_ptr(), nt.data_ptr(), wt.data_ptr()
    lo, up = wp, wp + 8 * n
    L, vp = G.lib(), ctypes.c_void_p

    def run(hay=hp, hay_count=64, needles=np_, needle_count=64, lower=lo, upper=up, key_type="uint32", reuse=False):
        ss.run_ptr(hay, hay_count, needles, needle_count, lower, upper, key_type, reuse)

    def raw(key_type):
        G.check(L.glu_sorted_search_run_ptr(ss._h, vp(hp), 64, vp(np_), 64, key_type, vp(lo), vp(up), 0, None))

    bad = [
        (lambda: G.check(L.glu_sorted_search_run_ptr(None, vp(hp), 64, vp(np_), 64, 0, vp(lo), vp(up), 0, None)), "search is NULL"),
        (lambda: G.check(L.glu_sorted_search_index_ptr(None, vp(hp), 64, 0, None)), "search is NULL"),
        (lambda: G.check(L.glu_sorted_search_prepare(None, 64, 0)), "search is NULL"),
        (lambda: G.check(L.glu_sorted_search_set_option(None, b"PATH", 0)), "search is NULL"),
        (lambda: G.check(L.glu_sorted_search_last(None, None, None, None)), "search is NULL"),
        (lambda: G.check(L.glu_sorted_search_create(None)), "out is NULL"),
        (lambda: run(hay=None), "Invalid hay buffer"),
        (lambda: ss.index_ptr(None, 64), "Invalid hay buffer"),
        (lambda: run(needles=None), "Invalid needles buffer"),
        (lambda: run(lower=None, upper=None), "out_lower and out_upper are both NULL"),
        (lambda: run(hay=hp + 2), "hay is not aligned"),
        (lambda: run(hay=hp + 4, key_type="uint64"), "hay is not aligned"),
        (lambda: ss.index_ptr(hp + 4, 64, "float64"), "hay is not aligned"),
        (lambda: run(needles=np_ + 1), "needles is not aligned"),
        (lambda: run(needles=np_ + 4, key_type="int64"), "needles is not aligned"),
        (lambda: run(lower=lo + 2), "out_lower is not aligned"),
        (lambda: run(upper=up + 1), "out_upper is not aligned"),
        (lambda: raw(6), "Invalid key type"),
        (lambda: raw(-1), "Invalid key type"),
        (lambda: G.check(L.glu_sorted_search_prepare(ss._h, 64, 6)), "Invalid key type"),
        (lambda: G.check(L.glu_sorted_search_index_ptr(ss._h, vp(hp), 64, 9, None)), "Invalid key type"),
        (lambda: run(hay_count=1 << 32), "hay_count below 2^32"),
        (lambda: ss.prepare(1 << 32), "hay_count below 2^32"),
        (lambda: ss.index_ptr(hp, 1 << 32), "hay_count below 2^32"),
        (lambda: run(needle_count=1 << 32), "needle_count below 2^32"),
        (lambda: run(lower=hp + 128), "out_lower overlaps hay"),
        (lambda: run(lower=np_ + 252), "out_lower overlaps needles"),
        (lambda: run(upper=hp - 4 * 63), "out_upper overlaps hay"),
        (lambda: run(upper=np_), "out_upper overlaps needles"),
        (lambda: run(upper=lo + 252), "out_upper overlaps out_lower"),
        (lambda: run(upper=lo), "out_upper overlaps out_lower"),
        (lambda: ss.set_option("PATH", 3), "PATH must be"),
        (lambda: ss.set_option("PATH", -1), "PATH must be"),
        (lambda: ss.set_option("TOP_ENTRIES", 15), "TOP_ENTRIES must lie"),
        (lambda: ss.set_option("TOP_ENTRIES", 8193), "TOP_ENTRIES must lie"),
        (lambda: ss.set_option("TOP_ENTRIES", 0), "TOP_ENTRIES must lie"),
        (lambda: ss.set_option("DIGIT_BITS", 8), "Unknown option"),
        (lambda: ss.set_option("path", 1), "Unknown option"),
        (lambda: G.check(L.glu_sorted_search_set_option(ss._h, None, 1)), "name is NULL"),
    ]
    assert len({m for _, m in bad}) == 21  # (the messages are distinct)
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    # a TOP_ENTRIES that one key width takes and the other does not is refused by the call of the other width
    ss.set_option("TOP_ENTRIES", 16)
    with pytest.raises(G.GluError) as e:
        run()
    assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT and "TOP_ENTRIES must lie in [32, 8192] for 4-byte keys" in e.value.message
    ss.set_option("TOP_ENTRIES", 8192)
    with pytest.raises(G.GluError) as e:
        run(key_type="uint64", hay_count=32, needle_count=32)
    assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT and "TOP_ENTRIES must lie in [16, 4096] for 8-byte keys" in e.value.message
    ss.set_option("TOP_ENTRIES", 32)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (ht.cpu().numpy().view(np.uint32) == hay).all() and (nt.cpu().numpy().view(np.uint32) == needles).all()
    # arrays that only touch are fine: the haystack is the middle of its buffer, out_lower ends where it begins, out_upper begins
    # where it ends; and no needles: nothing written
    part = hay[100:n - 100]
    for path in (DIRECT, INDEXED):
        ss.set_option("PATH", path)
        ss.run_ptr(hp + 400, n - 200, np_, 100, hp, hp + 4 * (n - 100), stream=stream())
        torch.cuda.synchronize()
        got = ht.cpu().numpy().view(np.uint32)
        assert (got[100:n - 100] == part).all()
        assert (got[:100] == np.searchsorted(part, needles[:100], "left")).all()
        assert (got[n - 100:] == np.searchsorted(part, needles[:100], "right")).all()
        ss.run_ptr(hp + 400, n - 200, None, 0, lo, up, stream=stream())
        assert ss.last() == ((DIRECT, 0, 0) if path == DIRECT else (INDEXED, 2, 1))
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all()


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one INDEXED call without reuse (the index kernel
    and the search kernel, on one stream) captured on a side stream is replayed on three haystack and needle contents in the same
    buffers: the launch sequence does not depend on the data."""
    import torch

    n, m = 100003, 20000
    rng = np.random.default_rng(90)
    ss = G.SortedSearch()
    ss.set_option("TOP_ENTRIES", 32)
    ss.set_option("PATH", INDEXED)
    ht = torch.empty(n, dtype=torch.int32, device="cuda")
    nt = torch.empty(m, dtype=torch.int32, device="cuda")
    lo = torch.empty(m, dtype=torch.int32, device="cuda")
    up = torch.empty(m, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def contents(spread):
        hay = np.sort(rng.integers(0, spread, n, dtype=np.uint32))
        return hay, rng.integers(0, min(spread + max(spread // 8, 2), 2 ** 32), m, dtype=np.uint32)

    def fill(hay, needles):
        ht.copy_(torch.from_numpy(hay.view(np.int32)))
        nt.copy_(torch.from_numpy(needles.view(np.int32)))
        lo.fill_(-1515870811)
        up.fill_(-1515870811)

    def verify(hay, needles):
        assert (lo.cpu().numpy().view(np.uint32) == np.searchsorted(hay, needles, "left")).all()
        assert (up.cpu().numpy().view(np.uint32) == np.searchsorted(hay, needles, "right")).all()

    def call(s):
        ss.run_ptr(ht.data_ptr(), n, nt.data_ptr(), m, lo.data_ptr(), up.data_ptr(), "uint32", False, s)

    with torch.cuda.stream(side):
        data = contents(2 ** 32)
        fill(*data)
        side.synchronize()
        ss.prepare(n, "uint32")
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert ss.last() == (INDEXED, 3, 2)
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for spread in (2 ** 32, 5000, 3):  # all keys different, twenty copies of every key, three keys
            data = contents(spread)
            fill(*data)
            graph.replay()
            side.synchronize()
            verify(*data)


def test_with_the_family(G):
    """Sort (key, value) pairs, key runs into a unique_keys array pre-filled with the largest key, then search 10 000 needles (half
    of them present) in all max_runs entries of it -- three calls on one stream with no host read in between.  A needle is found
    iff upper > lower, and the length of its run is offsets[lower + 1] - offsets[lower]: against a numpy group-by."""
    import torch

    rng = np.random.default_rng(70)
    n, distinct, max_runs = 200011, 9000, 9500  # (more unique keys than LDS holds: the search takes its index)
    alphabet = rng.choice(2 ** 31, distinct, replace=False).astype(np.uint32) * np.uint32(2)  # even keys
    keys = alphabet[rng.integers(0, distinct, n)]
    vals = np.arange(n, dtype=np.uint32)
    present, lengths = np.unique(keys, return_counts=True)
    needles = rng.permutation(np.concatenate([present[rng.integers(0, present.size, 5000)],
                                              alphabet[rng.integers(0, distinct, 5000)] + np.uint32(1)]))  # odd keys: absent
    kt = torch.from_numpy(keys.view(np.int32)).cuda()
    vt = torch.from_numpy(vals.view(np.int32)).cuda()
    unique = Array(np.full(max_runs, 0xFFFFFFFF, dtype=np.uint32))
    offsets, runs_n = Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4)
    na, lo, up = Array(needles), Array.poisoned(4 * needles.size), Array.poisoned(4 * needles.size)
    s = stream()
    ss = G.SortedSearch()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "uint32", s)
    G.KeyRuns().run_ptr(kt.data_ptr(), n, offsets.ptr, max_runs, runs_n.ptr, unique_keys_ptr=unique.ptr, stream=s)
    ss.run_ptr(unique.ptr, max_runs, na.ptr, needles.size, lo.ptr, up.ptr, stream=s)
    torch.cuda.synchronize()
    assert ss.last() == (INDEXED, 1, 2)
    assert int(runs_n.result(np.uint32)[0]) == present.size
    lower, upper, offs = lo.result(np.uint32), up.result(np.uint32), offsets.result(np.uint32)
    found = upper > lower
    assert (found == np.isin(needles, present)).all() and found.sum() == 5000
    assert (upper[found] == lower[found] + 1).all()
    joined = offs[lower[found] + 1] - offs[lower[found]]
    assert (joined == lengths[np.searchsorted(present, needles[found])]).all()
    assert (lower[~found] == np.searchsorted(present, needles[~found])).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_sorted_search_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
