"""GPU tests of merge (glu_merge_run_ptr): two sorted arrays of keys, with or without uint32 values, into one, stable.  The oracle is
always numpy: order = argsort(enc(A || B), kind="stable") on the keys as the sort encodes them (unsigned, in the sort's order);
the expected keys are (A || B)[order] compared as bit patterns, the expected values (A's iota || B's iota + 2^31)[order], so the side
and the place every output came from are visible.  Every comparison is `==`.  Every array the call writes sits inside an allocation
with poison in front of it and behind it, and is itself filled with poison first; the inputs are checked unchanged; last() is
checked against plan_merge.  The scheme is that of test_gpu_sorted_search.py."""
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
KEYS = {"uint32": np.uint32, "int32": np.uint32, "float32": np.uint32, "uint64": np.uint64, "int64": np.uint64, "float64": np.uint64}
B_VALS = 1 << 31  # B's values start here


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


def in_order(a):
    """`a` sorted in the sort's order (stable)."""
    return a[np.argsort(enc(a), kind="stable")]


def tile_of(G, key_type):
    return G.plan_merge(1, 1, key_type)[0]


def oracle(a, b):
    """(keys as bit patterns, values) of the stable sort of A || B by the encoded keys; values are A: iota, B: iota + 2^31."""
    ea, eb = enc(a), enc(b)
    assert (ea[1:] >= ea[:-1]).all() and (eb[1:] >= eb[:-1]).all(), "the test's inputs are not sorted"
    u = KEYS[str(a.dtype)]
    both = np.concatenate([a.view(u), b.view(u)])
    order = np.argsort(np.concatenate([ea, eb]), kind="stable")
    vals = np.concatenate([np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)])
    return both[order], vals[order]


def check_case(G, mg, a, b, with_vals=True, shifts=(0, 0, 0, 0, 0, 0), want=None, unsorted=False):
    """One call.  `a` and `b` of one of the six key types, sorted in the sort's order (unless `unsorted`: then only the poison, the
    inputs and last() are checked).  shifts: bytes behind a 16-byte boundary of a_keys, a_vals, b_keys, b_vals, out_keys, out_vals.
    Returns the oracle's (keys, values)."""
    import torch

    key_type = str(a.dtype)
    assert b.dtype == a.dtype
    u, kb, total = KEYS[key_type], a.dtype.itemsize, a.size + b.size
    av, bv = np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)
    ak, bk = Array(a.view(u), shifts[0]), Array(b.view(u), shifts[2])
    ava, bva = Array(av, shifts[1]), Array(bv, shifts[3])
    ok, ov = Array.poisoned(kb * total, shifts[4]), Array.poisoned(4 * total, shifts[5])
    for arr, s in zip((ak, ava, bk, bva, ok, ov), shifts):
        assert arr.ptr % 16 == s
    # a side of no elements passes NULL pointers
    mg.run_ptr(ak.ptr if a.size else None, ava.ptr if with_vals and a.size else None, a.size,
               bk.ptr if b.size else None, bva.ptr if with_vals and b.size else None, b.size,
               ok.ptr if total else None, ov.ptr if with_vals and total else None, key_type, stream())
    torch.cuda.synchronize()
    what = (key_type, a.size, b.size, with_vals, shifts)
    assert mg.last() == G.plan_merge(a.size, b.size, key_type, with_vals)[1:3], (what, mg.last())
    got_keys, got_vals = ok.result(u), ov.result(np.uint32)
    assert (ak.result(u) == a.view(u)).all() and (bk.result(u) == b.view(u)).all(), "the call wrote to its keys"
    assert (ava.result(np.uint32) == av).all() and (bva.result(np.uint32) == bv).all(), "the call wrote to its values"
    if not with_vals:
        assert (got_vals.view(np.uint8) == POISON).all(), (what, "keys only, and out_vals was written")
    if unsorted:
        return None
    want = want or oracle(a, b)
    bad = np.flatnonzero(got_keys != want[0])
    assert bad.size == 0, (what, "keys", int(bad[0]), int(got_keys[bad[0]]), int(want[0][bad[0]]))
    if with_vals:
        bad = np.flatnonzero(got_vals != want[1])
        assert bad.size == 0, (what, "values", int(bad[0]), int(got_vals[bad[0]]), int(want[1][bad[0]]))
    return want


def uniform(rng, n, dtype=np.uint32):
    return np.sort(rng.integers(0, 2 ** (8 * np.dtype(dtype).itemsize), n, dtype=dtype))


def test_tiny(G):
    mg = G.Merge()
    rng = np.random.default_rng(1)
    for na, nb in ((0, 0), (0, 1), (1, 0), (3, 5)):
        for with_vals in (True, False):
            check_case(G, mg, uniform(rng, na), uniform(rng, nb), with_vals)
    assert G.plan_merge(0, 0)[1:3] == (0, 0) and G.plan_merge(0, 1)[1:3] == (1, 2)
    for x, y, first in ((1, 2, 0), (2, 2, 0), (3, 2, B_VALS)):  # a < b, a == b (A first), a > b
        keys, vals = check_case(G, mg, np.array([x], dtype=np.uint32), np.array([y], dtype=np.uint32))
        assert vals[0] == first and keys.tolist() == sorted([x, y])


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_tile_boundaries(G, key_type):
    T = tile_of(G, key_type)
    rng = np.random.default_rng(T)
    mg = G.Merge()
    for total in (T - 1, T, T + 1, 2 * T, 3 * T + 17):
        for na in (0, 1, total // 2, total - 1, total):
            check_case(G, mg, uniform(rng, na, key_type), uniform(rng, total - na, key_type))
    assert mg.last() == (4, 2)


def test_ties(G):
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(3)
    mg = G.Merge()
    total = 4 * T + 5
    na = total // 2 + 7
    a = np.sort(rng.integers(0, 3, na)).astype(np.uint32) * np.uint32(0x40000001)
    b = np.sort(rng.integers(0, 3, total - na)).astype(np.uint32) * np.uint32(0x40000001)
    keys, vals = check_case(G, mg, a, b)
    for k in np.unique(keys):  # among equal keys: A's elements in their order, then B's in theirs
        v = vals[keys == k].astype(np.int64)
        assert (np.diff(v) > 0).all()
    check_case(G, mg, a, b, with_vals=False)
    same = np.full(3 * T, 77, dtype=np.uint32)
    keys, vals = check_case(G, mg, same, same.copy())
    assert (vals == np.concatenate([np.arange(3 * T), np.arange(3 * T) + B_VALS])).all()  # A's iota, then B's


def test_disjoint(G):
    """All of A below all of B, and the reverse: the splits sit at the ends of their ranges."""
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(4)
    mg = G.Merge()
    low = np.sort(rng.integers(0, 1 << 30, T + 3, dtype=np.uint32))
    high = np.sort(rng.integers(1 << 31, 1 << 32, 2 * T + 1, dtype=np.uint32))
    keys, vals = check_case(G, mg, low, high)
    assert (vals[:T + 3] < B_VALS).all() and (vals[T + 3:] >= B_VALS).all()
    keys, vals = check_case(G, mg, np.sort(high[:T + 3]), np.concatenate([low, low[-1:].repeat(T - 2)]))
    assert (vals[:2 * T + 1] >= B_VALS).all() and (vals[2 * T + 1:] < B_VALS).all()


def test_skewed(G):
    T = tile_of(G, "uint32")
    mg = G.Merge()
    long = np.repeat(np.arange(1000, 1000 + T, dtype=np.uint32), 5)  # (five copies of every key)
    dup = long[[7, T, 2 * T + 1, 3 * T, 5 * T - 1]]  # the short side equals duplicates of the long side
    for short in (np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.uint32) + np.uint32(1 << 20), dup):
        check_case(G, mg, short, long)
        check_case(G, mg, long, short)


def float_specials(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    top = 8 * np.dtype(dtype).itemsize - 1
    quiet = (u(0x7FC) << u(top - 11)) if dtype == np.float32 else (u(0x7FF8) << u(top - 15))
    nans = np.array([quiet | u(1), quiet | u(0x12345), (u(1) << u(top)) | quiet | u(1), (u(1) << u(top)) | quiet | u(0x12345)], dtype=u).view(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    return np.concatenate([np.array([-0.0, 0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(dtype).max, np.finfo(dtype).min], dtype=dtype), nans])


def typed_keys(rng, n, key_type):
    """n keys of the type with its specials among them (on both sides of a merge: ties across the sides), in the sort's order."""
    dtype = np.dtype(key_type)
    if dtype.kind == "f":
        special = float_specials(dtype.type)
        keys = (rng.integers(-3000, 3000, n) / 16.0).astype(dtype)
    else:
        info = np.iinfo(dtype)
        special = np.array([info.min, info.max, 0, 1] + ([-1] if dtype.kind == "i" else []), dtype=dtype)
        span = 20000 if dtype.itemsize == 4 else 20000 * 0x100000001
        keys = (rng.integers(-3000, 3000, n) if dtype.kind == "i" else rng.integers(0, 6000, n)).astype(dtype) * dtype.type(span // 6000)
    keys[rng.choice(n, 2 * special.size, replace=False)] = np.tile(special, 2)
    return in_order(keys)


@pytest.mark.parametrize("key_type", sorted(KEYS))
def test_every_key_type(G, key_type):
    """2T + 9 keys per side (T the tile of the key width) with the type's specials on both sides: +-0.0, +-inf, NaNs of both signs
    and two payloads, denormals; INT_MIN / INT_MAX; 0 / UINT_MAX."""
    T = tile_of(G, key_type)
    assert T == G.plan_merge(1, 1, key_type, False)[0] and (T == tile_of(G, "uint32")) == (np.dtype(key_type).itemsize == 4)
    rng = np.random.default_rng(len(key_type) + T)
    n = 2 * T + 9
    a, b = typed_keys(rng, n, key_type), typed_keys(rng, n, key_type)
    mg = G.Merge()
    keys, vals = check_case(G, mg, a, b)
    check_case(G, mg, a, b, with_vals=False)
    dtype = np.dtype(key_type)
    if dtype.kind == "f":  # -0.0 in front of +0.0, the NaNs at both ends, and every special of A in front of the same one of B
        typed = keys.view(dtype)
        zeros = np.flatnonzero(typed == 0)
        signs = np.signbit(typed[zeros])
        assert signs.sum() == 4 and (~signs).sum() >= 4 and (np.diff(signs.astype(np.int8)) <= 0).all()
        assert np.isnan(typed[:4]).all() and np.isnan(typed[-4:]).all() and np.isnan(typed).sum() == 16
        v = vals[:4].astype(np.int64)
        assert ((v < B_VALS).sum(), (v >= B_VALS).sum()) == (2, 2)


def test_keys_only(G):
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(7)
    mg = G.Merge()
    check_case(G, mg, uniform(rng, 2 * T + 100), uniform(rng, T - 50), with_vals=False)
    check_case(G, mg, uniform(rng, T + 1, np.uint64), uniform(rng, 3 * T, np.uint64), with_vals=False)


def test_alignment(G):
    """Each of the six arrays 4, 8 or 12 bytes behind a 16-byte boundary (8 for 8-byte keys), some in turn and all at once."""
    rng = np.random.default_rng(8)
    mg = G.Merge()
    T = tile_of(G, "uint32")
    a, b = uniform(rng, 2 * T + 5), uniform(rng, T + 11)
    want = check_case(G, mg, a, b)
    for shifts in ((4, 0, 0, 0, 0, 0), (0, 0, 12, 0, 0, 0), (0, 8, 0, 4, 0, 0), (0, 0, 0, 0, 4, 0), (0, 0, 0, 0, 0, 12), (0, 0, 0, 0, 8, 8),
                   (4, 8, 12, 4, 8, 12), (12, 12, 12, 12, 12, 12), (4, 4, 8, 8, 12, 4)):
        check_case(G, mg, a, b, shifts=shifts, want=want)
    check_case(G, mg, a, b, with_vals=False, shifts=(8, 0, 4, 0, 12, 0), want=want)
    T = tile_of(G, "uint64")
    a, b = uniform(rng, T + 3, np.uint64), uniform(rng, 2 * T + 2, np.uint64)
    want = check_case(G, mg, a, b)
    for shifts in ((8, 0, 0, 0, 0, 0), (0, 0, 0, 0, 8, 0), (0, 4, 8, 12, 0, 0), (8, 4, 8, 12, 8, 4), (8, 8, 8, 8, 8, 8)):
        check_case(G, mg, a, b, shifts=shifts, want=want)


@pytest.mark.parametrize("key_type", ["uint32", "float64"])
def test_many_tiles(G, key_type):
    """257 T + 9 outputs: 258 tiles, 259 tile boundaries, the partition kernel's second workgroup (the tile kernel takes one
    workgroup per tile, no loop)."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(9)
    total = 257 * T + 9
    na = total // 3
    if key_type == "uint32":
        a, b = uniform(rng, na), uniform(rng, total - na)
    else:
        a, b = np.sort(rng.standard_normal(na)), np.sort(rng.standard_normal(total - na))
    mg = G.Merge()
    check_case(G, mg, a, b)
    assert mg.last() == (258, 2)


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one call (the two kernels, on one stream) captured on
    a side stream is replayed on three contents of the same buffers with the same counts: the launch sequence does not depend on the
    data."""
    import torch

    T = tile_of(G, "uint32")
    na, nb = 20 * T + 3, 7 * T + 1
    rng = np.random.default_rng(90)
    mg = G.Merge()
    at, bt = torch.empty(na, dtype=torch.int32, device="cuda"), torch.empty(nb, dtype=torch.int32, device="cuda")
    avt = torch.arange(na, dtype=torch.int32, device="cuda")
    bvt = torch.from_numpy((np.arange(nb, dtype=np.uint32) + np.uint32(B_VALS)).view(np.int32)).cuda()
    ok, ov = torch.empty(na + nb, dtype=torch.int32, device="cuda"), torch.empty(na + nb, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def contents(spread):
        return np.sort(rng.integers(0, spread, na, dtype=np.uint32)), np.sort(rng.integers(0, spread, nb, dtype=np.uint32))

    def fill(a, b):
        at.copy_(torch.from_numpy(a.view(np.int32)))
        bt.copy_(torch.from_numpy(b.view(np.int32)))
        ok.fill_(-1515870811)
        ov.fill_(-1515870811)

    def verify(a, b):
        keys, vals = oracle(a, b)
        assert (ok.cpu().numpy().view(np.uint32) == keys).all()
        assert (ov.cpu().numpy().view(np.uint32) == vals).all()

    def call(s):
        mg.run_ptr(at.data_ptr(), avt.data_ptr(), na, bt.data_ptr(), bvt.data_ptr(), nb, ok.data_ptr(), ov.data_ptr(), "uint32", s)

    with torch.cuda.stream(side):
        data = contents(2 ** 32)
        fill(*data)
        side.synchronize()
        mg.prepare(na + nb, "uint32")
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert mg.last() == (28, 2)
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for spread in (2 ** 32, 5000, 3):  # all keys different, many copies of every key, three keys
            data = contents(spread)
            fill(*data)
            graph.replay()
            side.synchronize()
            verify(*data)


def test_argument_errors(G):
    """Mixed NULL value pointers, an output overlapping an input, a bad key type and the other cases the host can check: each
    INVALID_ARGUMENT with its own message, and a witness buffer (every output lies in it) shows that nothing was written."""
    import torch

    mg = G.Merge()
    n = 4096
    keys = np.arange(n, dtype=np.uint32)
    at, bt = torch.from_numpy(keys.view(np.int32).copy()).cuda(), torch.from_numpy(keys.view(np.int32).copy()).cuda()
    avt, bvt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    wt = torch.zeros(8 * n, dtype=torch.int32, device="cuda")  # the witness: out_keys, out_vals
    ap, bp, avp, bvp, wp = at.data_ptr(), bt.data_ptr(), avt.data_ptr(), bvt.data_ptr(), wt.data_ptr()
    okp, ovp = wp, wp + 16 * n
    L, vp = G.lib(), ctypes.c_void_p

    def run(a=ap, av=avp, na=64, b=bp, bv=bvp, nb=64, ok=okp, ov=ovp, key_type="uint32"):
        mg.run_ptr(a, av, na, b, bv, nb, ok, ov, key_type)

    def raw(key_type):
        G.check(L.glu_merge_run_ptr(mg._h, vp(ap), vp(avp), 64, vp(bp), vp(bvp), 64, vp(okp), vp(ovp), key_type, None))

    bad = [
        (lambda: G.check(L.glu_merge_run_ptr(None, vp(ap), vp(avp), 64, vp(bp), vp(bvp), 64, vp(okp), vp(ovp), 0, None)), "merge is NULL"),
        (lambda: G.check(L.glu_merge_prepare(None, 64, 0)), "merge is NULL"),
        (lambda: G.check(L.glu_merge_last(None, None, None)), "merge is NULL"),
        (lambda: G.check(L.glu_merge_create(None)), "out is NULL"),
        (lambda: run(av=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(bv=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(ov=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(av=None, bv=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(a=None), "Invalid a_keys buffer"),
        (lambda: run(b=None), "Invalid b_keys buffer"),
        (lambda: run(ok=None), "Invalid out_keys buffer"),
        (lambda: run(ok=ap), "out_keys overlaps a_keys"),
        (lambda: run(ok=ap + 252), "out_keys overlaps a_keys"),
        (lambda: run(ok=bp - 4 * 127), "out_keys overlaps b_keys"),
        (lambda: run(ok=avp), "out_keys overlaps a_vals"),
        (lambda: run(ov=bvp + 128), "out_vals overlaps b_vals"),
        (lambda: run(ov=bp), "out_vals overlaps b_keys"),
        (lambda: run(ov=okp + 4 * 127), "out_vals overlaps out_keys"),
        (lambda: raw(6), "Invalid key type"),
        (lambda: raw(-1), "Invalid key type"),
        (lambda: G.check(L.glu_merge_prepare(mg._h, 64, 9)), "Invalid key type"),
        (lambda: run(a=ap + 2), "a_keys is not aligned"),
        (lambda: run(b=bp + 4, key_type="int64"), "b_keys is not aligned"),
        (lambda: run(ok=okp + 4, key_type="float64"), "out_keys is not aligned"),
        (lambda: run(av=avp + 1), "a_vals is not aligned"),
        (lambda: run(bv=bvp + 2), "b_vals is not aligned"),
        (lambda: run(ov=ovp + 3), "out_vals is not aligned"),
        (lambda: run(na=1 << 31, nb=1 << 31), "a_count + b_count below 2^32"),
        (lambda: mg.prepare(1 << 32), "a_count + b_count below 2^32"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (at.cpu().numpy().view(np.uint32) == keys).all() and (bt.cpu().numpy().view(np.uint32) == keys).all()
    # arrays that only touch are fine: A and B are the two ends of one buffer, out_keys the middle
    big = torch.from_numpy(np.concatenate([keys[:100], np.zeros(164, dtype=np.uint32), keys[50:114]]).view(np.int32).copy()).cuda()
    mg.run_ptr(big.data_ptr(), None, 100, big.data_ptr() + 4 * 264, None, 64, big.data_ptr() + 400, None, "uint32", stream())
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint32)
    assert (got[:100] == keys[:100]).all() and (got[264:] == keys[50:114]).all()
    assert (got[100:264] == np.sort(np.concatenate([keys[:100], keys[50:114]]), kind="stable")).all()


@pytest.mark.parametrize("key_type", ["uint32", "float32"])
def test_with_the_family(G, key_type):
    """Two halves of 70 001 pairs each sorted by the library's typed sort, then merged, all on one stream with no host read in
    between: keys and values equal the library's sort of the whole array, bit for bit (the sort is stable and the first half's
    values lie below the second's, so both orders agree among equal keys)."""
    import torch

    half = 70001
    rng = np.random.default_rng(70 + len(key_type))
    dtype = np.dtype(key_type)
    if dtype.kind == "f":
        keys = (rng.integers(-20000, 20000, 2 * half) / 8.0).astype(dtype)
        special = float_specials(dtype.type)
        keys[rng.choice(2 * half, 4 * special.size, replace=False)] = np.tile(special, 4)
    else:
        keys = rng.integers(0, 50000, 2 * half).astype(dtype) * dtype.type(85899)
    vals = np.arange(2 * half, dtype=np.uint32)
    whole_k, whole_v = Array(keys.view(np.uint32)), Array(vals)
    ak, av = Array(keys[:half].view(np.uint32)), Array(vals[:half])
    bk, bv = Array(keys[half:].view(np.uint32)), Array(vals[half:])
    ok, ov = Array.poisoned(8 * half), Array.poisoned(8 * half)
    s = stream()
    sort, mg = G.RadixSort(), G.Merge()
    sort.sort_typed_ptr(whole_k.ptr, whole_v.ptr, 2 * half, key_type, s)
    sort.sort_typed_ptr(ak.ptr, av.ptr, half, key_type, s)
    sort.sort_typed_ptr(bk.ptr, bv.ptr, half, key_type, s)
    mg.run_ptr(ak.ptr, av.ptr, half, bk.ptr, bv.ptr, half, ok.ptr, ov.ptr, key_type, s)
    torch.cuda.synchronize()
    assert mg.last() == G.plan_merge(half, half, key_type)[1:3]
    want_k, want_v = whole_k.result(np.uint32), whole_v.result(np.uint32)
    order = np.argsort(enc(keys), kind="stable")
    assert (want_k == keys.view(np.uint32)[order]).all() and (want_v == vals[order]).all(), "the typed sort is not numpy's stable sort"
    assert (ok.result(np.uint32) == want_k).all()
    assert (ov.result(np.uint32) == want_v).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_merge_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_unsorted_input_stays_inside_its_arrays(G, key_type):
    """3 T shuffled keys per side (tests/test_merge_path.py shows on the host that every range stays inside its array whatever the
    keys hold): the poison around the outputs is intact, the inputs are unchanged, last() is the plan's; the output's contents are
    unspecified and not looked at."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(13)
    a = rng.integers(0, 1 << 31, 3 * T).astype(key_type)
    b = rng.integers(0, 1 << 31, 3 * T).astype(key_type)
    mg = G.Merge()
    check_case(G, mg, a, b, unsorted=True)
    check_case(G, mg, np.sort(a), b[::-1].copy(), shifts=(0, 4, 8, 12, 8, 4), unsorted=True)
