"""GPU tests of the set operations (glu_set_ops_run_ptr): union, intersection, difference and symmetric difference of two sorted
arrays of keys, with or without uint32 values.  The oracle is always numpy, on the keys as the sort encodes them (ea, eb: unsigned,
in the sort's order):
    ra = arange(na) - searchsorted(ea, ea, "left");  mb = searchsorted(eb, ea, "right") - searchsorted(eb, ea, "left")
    rb, ma likewise;  matchA = ra < mb;  matchB = rb < ma
    union: all of A, B & ~matchB;  intersection: A & matchA;  difference: A & ~matchA;  symmetric difference: A & ~matchA, B & ~matchB
    order = argsort(concat(ea, eb), kind="stable");  kept = order[concat(keepA, keepB)[order]]
The expected keys are (A || B)[kept] compared as bit patterns, the expected values (A's iota || B's iota + 2^31)[kept], so the side and
the place every output came from are visible.  Every comparison is `==`.  Every array the call writes sits inside an allocation with
poison in front of it and behind it, and is itself filled with poison first; the inputs are checked unchanged; last() is checked
against plan_set_ops.  The scheme is that of test_gpu_merge.py."""
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
OPS = ("union", "intersection", "difference", "symmetric_difference")


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
    return G.plan_set_ops(1, 1, key_type)[0]


def bound_of(op, na, nb):
    return {"union": na + nb, "symmetric_difference": na + nb, "difference": na, "intersection": min(na, nb)}[op]


def kept_of(ea, eb):
    """{op: the kept elements as indices into A || B, in the output's order}; ea, eb the encoded keys, sorted."""
    assert (ea[1:] >= ea[:-1]).all() and (eb[1:] >= eb[:-1]).all(), "the test's inputs are not sorted"
    na, nb = ea.size, eb.size
    ra = np.arange(na) - np.searchsorted(ea, ea, "left")
    mb = np.searchsorted(eb, ea, "right") - np.searchsorted(eb, ea, "left")
    rb = np.arange(nb) - np.searchsorted(eb, eb, "left")
    ma = np.searchsorted(ea, eb, "right") - np.searchsorted(ea, eb, "left")
    match_a, match_b = ra < mb, rb < ma
    no_a, no_b = np.zeros(na, bool), np.zeros(nb, bool)
    keep = {"union": (~no_a, ~match_b), "intersection": (match_a, no_b), "difference": (~match_a, no_b),
            "symmetric_difference": (~match_a, ~match_b)}
    order = np.argsort(np.concatenate([ea, eb]), kind="stable")
    return {op: order[np.concatenate(k)[order]] for op, k in keep.items()}


def oracle(a, b):
    """{op: (keys as bit patterns, values)}; values are A: iota, B: iota + 2^31.  Computed once per pair of inputs."""
    u = KEYS[str(a.dtype)]
    both = np.concatenate([a.view(u), b.view(u)])
    vals = np.concatenate([np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)])
    return {op: (both[k], vals[k]) for op, k in kept_of(enc(a), enc(b)).items()}


def check_case(G, so, op, a, b, with_vals=True, shifts=(0, 0, 0, 0, 0, 0, 0), want=None, max_out=None, count_only=False, unsorted=False):
    """One call.  `a` and `b` of one of the six key types, sorted in the sort's order (unless `unsorted`: then only the promise is
    checked).  shifts: bytes behind a 16-byte boundary of a_keys, a_vals, b_keys, b_vals, out_keys, out_vals, num_out.  max_out None:
    the operation's bound.  Returns (keys, values) of the oracle for this operation."""
    import torch

    key_type = str(a.dtype)
    assert b.dtype == a.dtype
    u, kb, na, nb = KEYS[key_type], a.dtype.itemsize, a.size, b.size
    bound = bound_of(op, na, nb)
    room = bound if max_out is None else max_out
    av, bv = np.arange(na, dtype=np.uint32), np.arange(nb, dtype=np.uint32) + np.uint32(B_VALS)
    ak, bk = Array(a.view(u), shifts[0]), Array(b.view(u), shifts[2])
    ava, bva = Array(av, shifts[1]), Array(bv, shifts[3])
    held = max(room, bound) + 3  # (the arrays hold more than may be written)
    ok, ov, num = Array.poisoned(kb * held, shifts[4]), Array.poisoned(4 * held, shifts[5]), Array.poisoned(4, shifts[6])
    for arr, s in zip((ak, ava, bk, bva, ok, ov, num), shifts):
        assert arr.ptr % 16 == s
    writes = not count_only and room > 0
    vals_too = with_vals and writes
    # a side of no elements passes NULL pointers; B's values only where the operation can write elements of B
    so.run_ptr(op, ak.ptr if na else None, ava.ptr if vals_too and na else None, na,
               bk.ptr if nb else None, bva.ptr if vals_too and nb and op in ("union", "symmetric_difference") else None, nb,
               None if count_only else ok.ptr, ov.ptr if vals_too else None, room, num.ptr, key_type, stream())
    torch.cuda.synchronize()
    what = (op, key_type, na, nb, with_vals, shifts, max_out, count_only)
    assert so.last() == G.plan_set_ops(na, nb, key_type, writes)[1:3], (what, so.last())
    got_keys, got_vals, got_num = ok.result(u), ov.result(np.uint32), int(num.result(np.uint32)[0])
    assert (ak.result(u) == a.view(u)).all() and (bk.result(u) == b.view(u)).all(), "the call wrote to its keys"
    assert (ava.result(np.uint32) == av).all() and (bva.result(np.uint32) == bv).all(), "the call wrote to its values"
    if not vals_too:
        assert (got_vals.view(np.uint8) == POISON).all(), (what, "no values, and out_vals was written")
    if unsorted:
        assert got_num <= bound, (what, got_num)
        n = min(got_num, room) if writes else 0
        assert (got_keys[n:].view(np.uint8) == POISON).all() and (got_vals[n:].view(np.uint8) == POISON).all(), (what, "written behind num_out")
        return None
    want = want or oracle(a, b)
    keys, vals = want[op]
    assert got_num == keys.size, (what, "num_out", got_num, keys.size)
    n = min(keys.size, room) if writes else 0
    bad = np.flatnonzero(got_keys[:n] != keys[:n])
    assert bad.size == 0, (what, "keys", int(bad[0]), int(got_keys[bad[0]]), int(keys[bad[0]]))
    assert (got_keys[n:].view(np.uint8) == POISON).all(), (what, "keys written behind min(S, max_out)")
    if vals_too:
        bad = np.flatnonzero(got_vals[:n] != vals[:n])
        assert bad.size == 0, (what, "values", int(bad[0]), int(got_vals[bad[0]]), int(vals[bad[0]]))
        assert (got_vals[n:].view(np.uint8) == POISON).all(), (what, "values written behind min(S, max_out)")
    return want


def all_ops(G, so, a, b, with_vals=True, **kw):
    want = oracle(a, b)
    for op in OPS:
        check_case(G, so, op, a, b, with_vals, want=want, **kw)
    return want


def uniform(rng, n, dtype=np.uint32, below=None):
    return np.sort(rng.integers(0, below or 2 ** (8 * np.dtype(dtype).itemsize), n, dtype=dtype))


def test_tiny(G):
    so = G.SetOps()
    rng = np.random.default_rng(1)
    for na, nb in ((0, 0), (0, 1), (1, 0), (3, 5)):
        for with_vals in (True, False):
            all_ops(G, so, uniform(rng, na, below=4), uniform(rng, nb, below=4), with_vals)
    assert G.plan_set_ops(0, 0)[1:] == (0, 1, 0) and G.plan_set_ops(0, 1)[1:] == (1, 4, 2 * 12 + 4)
    assert G.plan_set_ops(0, 1, "uint32", False)[1:3] == (1, 3)
    # single keys: a < b, a == b, a > b
    for x, y, sizes, union_vals in ((1, 2, (2, 0, 1, 2), [0, B_VALS]), (2, 2, (1, 1, 0, 0), [0]), (3, 2, (2, 0, 1, 2), [B_VALS, 0])):
        for with_vals in (True, False):
            want = all_ops(G, so, np.array([x], dtype=np.uint32), np.array([y], dtype=np.uint32), with_vals)
        assert tuple(want[op][0].size for op in OPS) == sizes
        assert want["union"][1].tolist() == union_vals


def test_runs_across_tiles(G):
    T = tile_of(G, "uint32")
    so = G.SetOps()
    long, short = np.full(3 * T, 77, dtype=np.uint32), np.full(2 * T + 5, 77, dtype=np.uint32)
    want = all_ops(G, so, long, short)
    assert (want["intersection"][1] == np.arange(2 * T + 5)).all()  # A's first 2T + 5
    assert (want["difference"][1] == np.arange(2 * T + 5, 3 * T)).all()  # A's last T - 5
    assert (want["union"][1] == np.arange(3 * T)).all()  # A alone
    assert (want["symmetric_difference"][1] == np.arange(2 * T + 5, 3 * T)).all()
    want = all_ops(G, so, short, long)
    assert (want["intersection"][1] == np.arange(2 * T + 5)).all() and want["difference"][1].size == 0
    assert (want["union"][1] == np.concatenate([np.arange(2 * T + 5), np.arange(2 * T + 5, 3 * T) + B_VALS])).all()
    assert (want["symmetric_difference"][1] == np.arange(2 * T + 5, 3 * T) + B_VALS).all()
    all_ops(G, so, long, short, with_vals=False)
    # an alphabet of 3, 4T + 5 elements in all
    rng = np.random.default_rng(3)
    total = 4 * T + 5
    na = total // 2 + 7
    a = np.sort(rng.integers(0, 3, na)).astype(np.uint32) * np.uint32(0x40000001)
    b = np.sort(rng.integers(0, 3, total - na)).astype(np.uint32) * np.uint32(0x40000001)
    all_ops(G, so, a, b)
    all_ops(G, so, a, b, with_vals=False)
    # a run that starts in the tile before and ends in the tile after, on both sides, of different lengths: the merged order is
    # [T - 40 small keys][A's run of T + 90][B's run of T + 30][large keys]
    low_a, low_b = np.arange(T // 2 - 20, dtype=np.uint32), np.arange(T // 2 - 20, dtype=np.uint32) + np.uint32(5)
    a = np.concatenate([low_a, np.full(T + 90, 1 << 20, dtype=np.uint32), np.arange(300, dtype=np.uint32) + np.uint32(1 << 21)])
    b = np.concatenate([low_b, np.full(T + 30, 1 << 20, dtype=np.uint32), np.arange(500, dtype=np.uint32) + np.uint32((1 << 21) + 100)])
    all_ops(G, so, a, b)
    all_ops(G, so, b, a)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_tile_boundaries(G, key_type):
    T = tile_of(G, key_type)
    assert T == {"uint32": 2816, "uint64": 1792}[key_type] == G.plan_merge(1, 1, key_type)[0]
    rng = np.random.default_rng(T)
    so = G.SetOps()
    for total in (T - 1, T, T + 1, 2 * T, 3 * T + 17):
        for na in (0, 1, total // 2, total - 1, total):
            all_ops(G, so, uniform(rng, na, key_type, 1 << 12), uniform(rng, total - na, key_type, 1 << 12))
    assert so.last() == (4, 4)


def test_disjoint_and_identical(G):
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(4)
    so = G.SetOps()
    low = np.sort(rng.integers(0, 1 << 30, T + 3, dtype=np.uint32))
    high = np.sort(rng.integers(1 << 31, 1 << 32, 2 * T + 1, dtype=np.uint32))
    want = all_ops(G, so, low, high)
    assert want["intersection"][0].size == 0 and want["union"][0].size == 3 * T + 4 and want["difference"][0].size == T + 3
    want = all_ops(G, so, high, low)
    assert want["intersection"][0].size == 0 and (want["union"][1][:T + 3] >= B_VALS).all()
    same = np.sort(rng.integers(0, 1 << 14, 2 * T + 7, dtype=np.uint32))
    want = all_ops(G, so, same, same.copy())
    assert (want["union"][1] == np.arange(same.size)).all() and (want["intersection"][1] == np.arange(same.size)).all()
    assert want["difference"][0].size == 0 and want["symmetric_difference"][0].size == 0
    all_ops(G, so, same, same.copy(), with_vals=False)


def float_specials(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    top = 8 * np.dtype(dtype).itemsize - 1
    quiet = (u(0x7FC) << u(top - 11)) if dtype == np.float32 else (u(0x7FF8) << u(top - 15))
    nans = np.array([quiet | u(1), quiet | u(0x12345), (u(1) << u(top)) | quiet | u(1), (u(1) << u(top)) | quiet | u(0x12345)], dtype=u).view(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    return np.concatenate([np.array([-0.0, 0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(dtype).max, np.finfo(dtype).min], dtype=dtype), nans])


def typed_keys(rng, n, key_type):
    """n keys of the type with its specials among them (on both sides: ties across the sides), in the sort's order."""
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
    rng = np.random.default_rng(len(key_type) + T)
    n = 2 * T + 9
    a, b = typed_keys(rng, n, key_type), typed_keys(rng, n, key_type)
    so = G.SetOps()
    all_ops(G, so, a, b)
    all_ops(G, so, a, b, with_vals=False)
    dtype = np.dtype(key_type)
    if dtype.kind == "f":
        # -0.0 and +0.0 are not matched with each other; a NaN matches only the NaN with the same bits
        u = KEYS[key_type]
        sp = float_specials(dtype.type)
        nans = sp[8:]
        a = in_order(np.concatenate([np.array([-0.0, -0.0, 1.5], dtype=dtype), nans[[0, 2]]]))  # (concatenate keeps the NaNs' bits)
        b = in_order(np.concatenate([np.array([0.0, 1.5], dtype=dtype), nans[[1, 2, 2]]]))
        want = all_ops(G, so, a, b)
        inter = want["intersection"][0]
        assert sorted(inter.tolist()) == sorted(np.concatenate([np.array([1.5], dtype=dtype), nans[[2]]]).view(u).tolist())
        diff = want["difference"][0]
        assert sorted(diff.tolist()) == sorted(np.concatenate([np.array([-0.0, -0.0], dtype=dtype), nans[[0]]]).view(u).tolist())
        assert want["union"][0].size == 8 and want["symmetric_difference"][0].size == 6


def test_max_out_and_count_only(G):
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(6)
    so = G.SetOps()
    a, b = uniform(rng, 2 * T + 100, below=1 << 13), uniform(rng, T + 50, below=1 << 13)
    want = oracle(a, b)
    for op in OPS:
        S = want[op][0].size
        assert 1 < S < bound_of(op, a.size, b.size)
        for max_out in (0, 1, S - 1, S, S + 1):
            for with_vals in (True, False):
                check_case(G, so, op, a, b, with_vals, want=want, max_out=max_out)
        check_case(G, so, op, a, b, False, want=want, count_only=True)
        check_case(G, so, op, a, b, False, want=want, count_only=True, max_out=5)
    a64, b64 = uniform(rng, T, np.uint64, 1 << 12), uniform(rng, T + 9, np.uint64, 1 << 12)
    want = oracle(a64, b64)
    for op in OPS:
        S = want[op][0].size
        for max_out in (0, S - 1, S + 1):
            check_case(G, so, op, a64, b64, want=want, max_out=max_out)


def test_alignment(G):
    """Each of the six arrays and num_out 4, 8 or 12 bytes behind a 16-byte boundary (8 for 8-byte keys), in turn and all at once;
    and inputs whose S differ by 1, 2 and 3: the output tiles start at offsets that follow from the data."""
    rng = np.random.default_rng(8)
    so = G.SetOps()
    T = tile_of(G, "uint32")
    a, b = uniform(rng, 2 * T + 5, below=1 << 13), uniform(rng, T + 11, below=1 << 13)
    want = oracle(a, b)
    turns = [tuple(s if i == j else 0 for i in range(7)) for j, s in enumerate((4, 8, 12, 4, 8, 12, 4))]
    for shifts in turns + [(0, 0, 0, 0, 12, 4, 8), (0, 0, 8, 8, 0, 0, 0), (4, 8, 12, 4, 8, 12, 4), (12, 12, 12, 12, 12, 12, 12), (8, 4, 4, 12, 4, 8, 12)]:
        for op in OPS:
            check_case(G, so, op, a, b, shifts=shifts, want=want)
    for op in OPS:
        check_case(G, so, op, a, b, with_vals=False, shifts=(8, 0, 4, 0, 12, 0, 8), want=want)
    # S differs by 1, 2, 3: three keys of A alone in front of everything, dropped one by one (they are in the first tile; the
    # outputs of every later tile move)
    a3, b3 = np.concatenate([np.array([1, 2, 3], dtype=np.uint32), a + np.uint32(10)]), b + np.uint32(10)
    sizes = set()
    for drop in (0, 1, 2, 3):
        want_d = oracle(a3[drop:], b3)
        sizes.add(want_d["union"][0].size % 4)
        for op in OPS:
            check_case(G, so, op, a3[drop:], b3, shifts=(0, 0, 0, 0, 4, 8, 0), want=want_d)
    assert sizes == {0, 1, 2, 3}
    T = tile_of(G, "uint64")
    a, b = uniform(rng, T + 3, np.uint64, 1 << 12), uniform(rng, 2 * T + 2, np.uint64, 1 << 12)
    want = oracle(a, b)
    for shifts in ((8, 0, 0, 0, 0, 0, 0), (0, 0, 8, 0, 0, 0, 0), (0, 0, 0, 0, 8, 0, 0), (0, 4, 0, 12, 0, 8, 4), (8, 4, 8, 12, 8, 4, 12), (8, 8, 8, 8, 8, 8, 8)):
        for op in OPS:
            check_case(G, so, op, a, b, shifts=shifts, want=want)
    a3, b3 = np.concatenate([np.array([1, 2, 3], dtype=np.uint64), a + np.uint64(10)]), b + np.uint64(10)
    for drop in (1, 2, 3):
        all_ops(G, so, a3[drop:], b3, shifts=(0, 0, 0, 0, 8, 4, 0))


@pytest.mark.parametrize("key_type", ["uint32", "float64"])
def test_many_tiles(G, key_type):
    """257 T + 9 elements in all: 258 tiles, 259 tile boundaries, the bounds kernel's second workgroup."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(9)
    total = 257 * T + 9
    na = total // 3
    if key_type == "uint32":
        a, b = uniform(rng, na, below=1 << 19), uniform(rng, total - na, below=1 << 19)
    else:
        a, b = np.sort(rng.integers(-1 << 18, 1 << 18, na) / 4.0), np.sort(rng.integers(-1 << 18, 1 << 18, total - na) / 4.0)
    so = G.SetOps()
    all_ops(G, so, a, b)
    assert so.last() == (258, 4)


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one captured union and one captured intersection (on
    one stream) are replayed on three contents of the same buffers with the same counts: the launch sequence does not depend on the
    data, although the number of outputs does."""
    import torch

    T = tile_of(G, "uint32")
    na, nb = 20 * T + 3, 7 * T + 1
    rng = np.random.default_rng(90)
    so_u, so_i = G.SetOps(), G.SetOps()
    at, bt = torch.empty(na, dtype=torch.int32, device="cuda"), torch.empty(nb, dtype=torch.int32, device="cuda")
    avt = torch.arange(na, dtype=torch.int32, device="cuda")
    bvt = torch.from_numpy((np.arange(nb, dtype=np.uint32) + np.uint32(B_VALS)).view(np.int32)).cuda()
    outs = {op: [torch.empty(na + nb, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.empty(1, dtype=torch.int32, device="cuda")]
            for op in ("union", "intersection")}
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    POISON32 = -1515870811

    def contents(spread):
        return np.sort(rng.integers(0, spread, na, dtype=np.uint32)), np.sort(rng.integers(0, spread, nb, dtype=np.uint32))

    def fill(a, b):
        at.copy_(torch.from_numpy(a.view(np.int32)))
        bt.copy_(torch.from_numpy(b.view(np.int32)))
        for ts in outs.values():
            for t in ts:
                t.fill_(POISON32)

    def verify(a, b):
        want = oracle(a, b)
        sizes = []
        for op, (ok, ov, num) in outs.items():
            keys, vals = want[op]
            sizes.append(keys.size)
            assert int(num.cpu().numpy().view(np.uint32)[0]) == keys.size
            assert (ok.cpu().numpy().view(np.uint32)[:keys.size] == keys).all() and (ov.cpu().numpy().view(np.uint32)[:keys.size] == vals).all()
            assert (ok.cpu().numpy()[keys.size:] == POISON32).all() and (ov.cpu().numpy()[keys.size:] == POISON32).all()
        return tuple(sizes)

    def call(s):
        for so, op in ((so_u, "union"), (so_i, "intersection")):
            ok, ov, num = outs[op]
            so.run_ptr(op, at.data_ptr(), avt.data_ptr(), na, bt.data_ptr(), bvt.data_ptr(), nb, ok.data_ptr(), ov.data_ptr(), na + nb,
                       num.data_ptr(), "uint32", s)

    with torch.cuda.stream(side):
        data = contents(2 ** 32)
        fill(*data)
        side.synchronize()
        so_u.prepare(na + nb, "uint32")
        so_i.prepare(na + nb, "uint32")
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert so_u.last() == (28, 4) and so_i.last() == (28, 4)
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        seen = set()
        for spread in (2 ** 32, 5000, 3):  # all keys different, many copies of every key, three keys
            data = contents(spread)
            fill(*data)
            graph.replay()
            side.synchronize()
            seen.add(verify(*data))
        assert len(seen) == 3  # (S differed each time)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_unsorted_input_stays_inside_its_arrays(G, key_type):
    """3 T shuffled keys per side, and one side sorted with the other reversed (tests/test_set_ops_path.py shows on the host that every
    index stays inside whatever the keys hold): the poison around the outputs is intact, the inputs are unchanged, num_out is at
    most the bound and nothing is written at or behind out[num_out]; the contents are unspecified and not looked at."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(13)
    a = rng.integers(0, 1 << 10, 3 * T).astype(key_type)
    b = rng.integers(0, 1 << 10, 3 * T).astype(key_type)
    so = G.SetOps()
    for op in OPS:
        check_case(G, so, op, a, b, unsorted=True)
        check_case(G, so, op, np.sort(a), np.sort(b)[::-1].copy(), shifts=(0, 4, 8, 12, 8, 4, 12), unsorted=True)
        check_case(G, so, op, np.sort(a)[::-1].copy(), np.sort(b), with_vals=False, shifts=(8, 0, 0, 0, 8, 0, 4), unsorted=True)
    # a short B that A matches again and again: the length stays at the bound
    check_case(G, so, "intersection", np.tile(np.array([5, 9], dtype=key_type), T), np.array([5], dtype=key_type), unsorted=True)


def test_argument_errors(G):
    """Every refusal the host can make: each INVALID_ARGUMENT with its own message, and a witness buffer (every output lies in it)
    shows that nothing was written.  Arrays that merely touch are accepted."""
    import torch

    so = G.SetOps()
    n = 4096
    keys = np.arange(n, dtype=np.uint32)
    at, bt = torch.from_numpy(keys.view(np.int32).copy()).cuda(), torch.from_numpy(keys.view(np.int32).copy()).cuda()
    avt, bvt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    wt = torch.zeros(8 * n + 16, dtype=torch.int32, device="cuda")  # the witness: out_keys, out_vals, num_out
    ap, bp, avp, bvp, wp = at.data_ptr(), bt.data_ptr(), avt.data_ptr(), bvt.data_ptr(), wt.data_ptr()
    okp, ovp, nump = wp, wp + 16 * n, wp + 32 * n
    L, vp = G.lib(), ctypes.c_void_p

    def run(op="union", a=ap, av=avp, na=64, b=bp, bv=bvp, nb=64, ok=okp, ov=ovp, max_out=128, num=nump, key_type="uint32"):
        so.run_ptr(op, a, av, na, b, bv, nb, ok, ov, max_out, num, key_type)

    def raw(op, key_type, handle=so._h):
        G.check(L.glu_set_ops_run_ptr(handle, op, vp(ap), vp(avp), 64, vp(bp), vp(bvp), 64, vp(okp), vp(ovp), 128, vp(nump), key_type, None))

    bad = [
        (lambda: raw(0, 0, None), "set_ops is NULL"),
        (lambda: G.check(L.glu_set_ops_prepare(None, 64, 0)), "set_ops is NULL"),
        (lambda: G.check(L.glu_set_ops_last(None, None, None)), "set_ops is NULL"),
        (lambda: G.check(L.glu_set_ops_create(None)), "out is NULL"),
        (lambda: run(a=None), "Invalid a_keys buffer"),
        (lambda: run(b=None), "Invalid b_keys buffer"),
        (lambda: run(num=None), "Invalid num_out pointer"),
        (lambda: run(av=None), "a_vals and out_vals must both be given or both be NULL"),
        (lambda: run(ov=None), "a_vals and out_vals must both be given or both be NULL"),
        (lambda: run("intersection", ov=None, bv=None), "a_vals and out_vals must both be given or both be NULL"),
        (lambda: run(bv=None), "b_vals is required"),
        (lambda: run("symmetric_difference", bv=None), "b_vals is required"),
        (lambda: run(ok=None), "out_vals needs out_keys"),
        (lambda: run(max_out=0), "out_vals needs out_keys"),
        (lambda: raw(4, 0), "op must be one of GLU_SET_UNION"),
        (lambda: raw(-1, 0), "op must be one of GLU_SET_UNION"),
        (lambda: raw(0, 6), "Invalid key type"),
        (lambda: raw(0, -1), "Invalid key type"),
        (lambda: G.check(L.glu_set_ops_prepare(so._h, 64, 9)), "Invalid key type"),
        (lambda: G.check(L.glu_set_ops_plan(1, 1, 6, 1, None, None, None, None)), "Invalid key type"),
        (lambda: run(a=ap + 2), "a_keys is not aligned"),
        (lambda: run(b=bp + 4, key_type="int64"), "b_keys is not aligned"),
        (lambda: run(ok=okp + 4, key_type="float64"), "out_keys is not aligned"),
        (lambda: run(av=avp + 1), "a_vals is not aligned"),
        (lambda: run(bv=bvp + 2), "b_vals is not aligned"),
        (lambda: run(ov=ovp + 3), "out_vals is not aligned"),
        (lambda: run(num=nump + 2), "num_out is not aligned"),
        (lambda: run(na=1 << 31, nb=1 << 31), "a_count + b_count below 2^32"),
        (lambda: run(na=1 << 32, nb=0), "a_count + b_count below 2^32"),
        (lambda: so.prepare(1 << 32), "a_count + b_count below 2^32"),
        (lambda: G.plan_set_ops(1 << 31, 1 << 31), "a_count + b_count below 2^32"),
        (lambda: run(max_out=1 << 32), "max_out must be below 2^32"),
        (lambda: run(ok=ap), "out_keys overlaps a_keys"),
        (lambda: run(ok=ap + 252), "out_keys overlaps a_keys"),
        (lambda: run(ok=bp - 4 * 127), "out_keys overlaps b_keys"),
        (lambda: run("intersection", ok=ap - 4 * 63), "out_keys overlaps a_keys"),
        (lambda: run(ok=avp), "out_keys overlaps a_vals"),
        (lambda: run(ov=bvp + 128), "out_vals overlaps b_vals"),
        (lambda: run(ov=bp), "out_vals overlaps b_keys"),
        (lambda: run(ov=okp + 4 * 127), "out_vals overlaps out_keys"),
        (lambda: run(num=ap + 4 * 63), "num_out overlaps a_keys"),
        (lambda: run(num=bvp), "num_out overlaps b_vals"),
        (lambda: run(num=okp + 4 * 127), "num_out overlaps out_keys"),
        (lambda: run(num=ovp), "num_out overlaps out_vals"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (at.cpu().numpy().view(np.uint32) == keys).all() and (bt.cpu().numpy().view(np.uint32) == keys).all()
    # arrays that only touch are fine: A and B are the two ends of one buffer, out_keys the middle (the union's bound: all 164),
    # num_out the word behind B
    big = torch.from_numpy(np.concatenate([keys[:100], np.zeros(164, dtype=np.uint32), keys[50:114], [7]]).astype(np.uint32).view(np.int32).copy()).cuda()
    so.run_ptr("union", big.data_ptr(), None, 100, big.data_ptr() + 4 * 264, None, 64, big.data_ptr() + 400, None, 164,
               big.data_ptr() + 4 * 328, "uint32", stream())
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint32)
    assert (got[:100] == keys[:100]).all() and (got[264:328] == keys[50:114]).all() and got[328] == 114
    assert (got[100:214] == keys[:114]).all() and (got[214:264] == 0).all()
    # intersection and difference ignore b_vals: NULL is fine, and so is one that overlaps an output
    run("intersection", bv=None)
    run("difference", bv=ovp)
    # an intersection's outputs are min(a_count, b_count) long: out_keys may end where A begins
    run("intersection", a=ap + 4 * 64, ok=ap, ov=ovp, max_out=4096)
    torch.cuda.synchronize()
    assert int(wt.cpu().numpy().view(np.uint32)[8 * n]) == 0  # (keys 64 .. 127 of A, keys 0 .. 63 of B: nothing in both)
    assert (at.cpu().numpy().view(np.uint32) == keys).all()


@pytest.mark.parametrize("key_type", ["uint32", "float32"])
def test_with_the_family(G, key_type):
    """Two arrays of 70 001 pairs each sorted by the library's typed sort, then all four operations on one stream with no host read in
    between: the results equal the oracle on the sorted arrays.  Then the unique keys of both (key runs) intersected: numpy's
    intersect1d on the encoded keys."""
    import torch

    n = 70001
    rng = np.random.default_rng(70 + len(key_type))
    dtype = np.dtype(key_type)
    if dtype.kind == "f":
        a, b = ((rng.integers(-20000, 20000, n) / 8.0).astype(dtype) for _ in range(2))
        special = float_specials(dtype.type)
        a[rng.choice(n, 2 * special.size, replace=False)] = np.tile(special, 2)
        b[rng.choice(n, special.size, replace=False)] = special
    else:
        a, b = (rng.integers(0, 50000, n).astype(dtype) * dtype.type(85899) for _ in range(2))
    av, bv = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) + np.uint32(B_VALS)
    ak, ava, bk, bva = Array(a.view(np.uint32)), Array(av), Array(b.view(np.uint32)), Array(bv)
    outs = {op: (Array.poisoned(8 * n), Array.poisoned(8 * n), Array.poisoned(4)) for op in OPS}
    s = stream()
    sort = G.RadixSort()
    objects = {op: G.SetOps() for op in OPS}
    sort.sort_typed_ptr(ak.ptr, ava.ptr, n, key_type, s)
    sort.sort_typed_ptr(bk.ptr, bva.ptr, n, key_type, s)
    for op in OPS:
        ok, ov, num = outs[op]
        objects[op].run_ptr(op, ak.ptr, ava.ptr, n, bk.ptr, bva.ptr, n, ok.ptr, ov.ptr, 2 * n, num.ptr, key_type, s)
    torch.cuda.synchronize()
    sa, sb, sav, sbv = ak.result(np.uint32).view(dtype), bk.result(np.uint32).view(dtype), ava.result(np.uint32), bva.result(np.uint32)
    assert (enc(sa) == np.sort(enc(a))).all() and (enc(sb) == np.sort(enc(b))).all(), "the typed sort did not sort"
    kept = kept_of(enc(sa), enc(sb))
    both_k, both_v = np.concatenate([sa.view(np.uint32), sb.view(np.uint32)]), np.concatenate([sav, sbv])
    for op in OPS:
        ok, ov, num = outs[op]
        S = kept[op].size
        assert int(num.result(np.uint32)[0]) == S
        assert (ok.result(np.uint32)[:S] == both_k[kept[op]]).all() and (ov.result(np.uint32)[:S] == both_v[kept[op]]).all()
        assert (ok.result(np.uint8)[4 * S:] == POISON).all() and (ov.result(np.uint8)[4 * S:] == POISON).all()
    # the unique keys of both sides, then their intersection
    runs = G.KeyRuns()
    uniq, counts = [], []
    for keys in (ak, bk):
        offs, u, num = Array.poisoned(4 * (n + 1)), Array.poisoned(4 * n), Array.poisoned(4)
        runs.run_ptr(keys.ptr, n, offs.ptr, n, num.ptr, u.ptr, stream=s)
        torch.cuda.synchronize()
        uniq.append(u)
        counts.append(int(num.result(np.uint32)[0]))
    ok, num = Array.poisoned(4 * n), Array.poisoned(4)
    objects["intersection"].run_ptr("intersection", uniq[0].ptr, None, counts[0], uniq[1].ptr, None, counts[1], ok.ptr, None, n, num.ptr, key_type, s)
    torch.cuda.synchronize()
    want = np.intersect1d(enc(a), enc(b))
    S = int(num.result(np.uint32)[0])
    assert S == want.size
    assert (enc(ok.result(np.uint32)[:S].view(dtype)) == want).all()


def test_past_2_31(G):
    """A is an iota of 2^31 + T + 3 uint32 keys (A[i] = i), B every 2^20-th value below 2^31 and three values behind 2^31: the
    intersection is B, the difference is A without B's values; indices and ranks past 2^31, an output past 8 GiB.  Keys only, both
    calls prepared, verified on the device with torch."""
    import gc

    import torch

    T = tile_of(G, "uint32")
    N = (1 << 31) + T + 3
    guard = T
    need = 2 * 4 * (N + 2 * guard) + (10 << 30)
    assert need <= 40 << 30, "no test may need more than 40 GiB"
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %d GiB of free HBM" % (need >> 30))
    CH = 1 << 27
    b_host = np.concatenate([np.arange(2048, dtype=np.int64) << 20, [(1 << 31) + 1, (1 << 31) + T, (1 << 31) + T + 2]])
    nb = b_host.size
    bt64 = torch.from_numpy(b_host).cuda()
    bt = torch.from_numpy(b_host.astype(np.uint32).view(np.int32)).cuda()
    at = torch.empty(N, dtype=torch.int32, device="cuda")
    for lo in range(0, N, CH):
        hi = min(N, lo + CH)
        at[lo:hi] = torch.arange(lo, hi, dtype=torch.int64, device="cuda").to(torch.int32)  # (wraps: the bits of the uint32)
    P32 = -1515870811
    out_d = torch.full((N + 2 * guard,), P32, dtype=torch.int32, device="cuda")
    out_i = torch.full((nb + 2 * guard,), P32, dtype=torch.int32, device="cuda")
    nums = torch.full((2,), P32, dtype=torch.int32, device="cuda")
    so_d, so_i = G.SetOps(), G.SetOps()
    so_d.prepare(N + nb)
    so_i.prepare(N + nb)
    # a stream of the caller's that waits for the fills above (they were made on the device and are not waited for by the host)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = side.cuda_stream
        so_d.run_ptr("difference", at.data_ptr(), None, N, bt.data_ptr(), None, nb, out_d.data_ptr() + 4 * guard, None, N, nums.data_ptr(), "uint32", s)
        so_i.run_ptr("intersection", at.data_ptr(), None, N, bt.data_ptr(), None, nb, out_i.data_ptr() + 4 * guard, None, nb, nums.data_ptr() + 4, "uint32", s)
    side.synchronize()
    torch.cuda.synchronize()
    assert so_d.last() == G.plan_set_ops(N, nb)[1:3] and so_i.last() == so_d.last()
    assert nums.cpu().numpy().view(np.uint32).tolist() == [N - nb, nb]
    assert bool((out_i[:guard] == P32).all()) and bool((out_i[guard + nb:] == P32).all())
    assert bool(((out_i[guard:guard + nb].to(torch.int64) & 0xFFFFFFFF) == bt64).all())
    assert bool((out_d[:guard] == P32).all()) and bool((out_d[guard + N - nb:] == P32).all()), "written outside out[0 .. S)"
    r = 0
    for lo in range(0, N, CH):
        hi = min(N, lo + CH)
        v = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        at_b = torch.searchsorted(bt64, v).clamp_(max=nb - 1)
        keep = v[bt64[at_b] != v]
        k = keep.numel()
        assert bool(((out_d[guard + r:guard + r + k].to(torch.int64) & 0xFFFFFFFF) == keep).all()), "the difference differs in the chunk at %d" % lo
        r += k
        del v, at_b, keep
    assert r == N - nb
    assert bool(((at[-CH:].to(torch.int64) & 0xFFFFFFFF) == torch.arange(N - CH, N, dtype=torch.int64, device="cuda")).all()), "the call wrote to A"
    del so_d, so_i, at, bt, bt64, out_d, out_i, nums
    gc.collect()
    torch.cuda.empty_cache()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_set_ops_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
