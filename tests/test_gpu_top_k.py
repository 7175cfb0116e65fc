"""GPU tests of top-k (glu_top_k_run_ptr): the k smallest or largest keys and their indices by a radix select, bit for bit against
numpy.argsort(code(keys), kind="stable")[:k], where code is the sort's key code (complemented for largest): boundaries of the tiles
and of k, ties at the threshold, the order of floats, both paths at small sizes, the output contract, refusals, capture, determinism,
indices past 2^31, the operator among the family, and the C++ program."""
import gc
import os
import subprocess

import numpy as np
import pytest

from test_top_k_pick import DTYPES, key_code

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
POISON = 0xA5
POISON32 = 0xA5A5A5A5
AUTO, CANDIDATES, FULL = 0, 1, 2


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
        host = np.concatenate([np.full(self.front, POISON, dtype=np.uint8), d.view(np.uint8).ravel(), np.full(GUARD, POISON, dtype=np.uint8)])
        self.t = torch.from_numpy(host).cuda()
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


def sync():
    import torch

    torch.cuda.synchronize()


def bits_of(a):
    return a.view("uint%d" % (8 * a.dtype.itemsize))


def expected(keys, k, largest, sorted_):
    head = np.argsort(key_code(keys, largest), kind="stable")[:k]
    return head if sorted_ else np.sort(head)


def check_case(G, top, keys, k, largest=False, sorted_=True, shift=0, with_keys=True, with_indices=True, with_kth=True, room=5, ka=None):
    """One call on `keys` and everything the contract says of it; returns read_last()."""
    import torch

    n, kb, name = keys.size, keys.dtype.itemsize, keys.dtype.name
    ka = ka or Array(keys, shift)
    ok, oi, ot = Array.poisoned((k + room) * kb), Array.poisoned((k + room) * 4), Array.poisoned(kb)
    top.run_ptr(ka.ptr, n, k, ok.ptr if with_keys else None, oi.ptr if with_indices else None, ot.ptr if with_kth else None, key_type=name,
                largest=largest, sorted=sorted_, stream=stream())
    torch.cuda.synchronize()
    last = top.read_last()
    want = expected(keys, k, largest, sorted_)
    case = (name, n, k, largest, sorted_, shift)
    got_k, got_i, got_t = ok.result(bits_of(keys).dtype), oi.result(np.uint32), ot.result(bits_of(keys).dtype)
    if with_keys:
        assert (got_k[:k] == bits_of(keys)[want]).all(), case
    if with_indices:
        assert (got_i[:k] == want).all(), case
    assert (ok.result(np.uint8)[(k if with_keys else 0) * kb:] == POISON).all(), case  # nothing behind entry k
    assert (oi.result(np.uint8)[(k if with_indices else 0) * 4:] == POISON).all(), case
    if with_kth and k:
        code = key_code(keys, largest)
        kth = np.argsort(code, kind="stable")[k - 1]
        assert got_t[0] == bits_of(keys)[kth], case
        assert code[kth] == np.partition(code, k - 1)[k - 1], case
        assert last["ties"] == k - int((code < code[kth]).sum()), case
    else:
        assert (ot.result(np.uint8) == POISON).all(), case
    assert (ka.result(bits_of(keys).dtype) == bits_of(keys)).all(), "top-k wrote to its input"
    arrays = with_keys or with_indices
    if k:
        assert last["kernels"] == G.plan_top_k(n, k, name, sorted=sorted_, with_arrays=arrays, **getattr(top, "plan_options", {}))["kernels"], case
    else:
        assert last == {"path": 0, "candidates": 0, "ties": 0, "kernels": 0}, case
    return last


def with_options(G, path, cand_capacity):
    """A TopK under these options, which check_case passes on to the plan."""
    top = G.TopK({"PATH": path, "CAND_CAPACITY": cand_capacity})
    top.plan_options = {"path": path, "cand_capacity": cand_capacity}
    return top


def random_keys(rng, dtype, n):
    """Every bit pattern of the top half of the word, duplicates among them (floats: NaNs and infinities of both signs too)."""
    dt = np.dtype(dtype)
    u = np.dtype("uint%d" % (8 * dt.itemsize))
    width = 8 * dt.itemsize
    return ((rng.integers(0, 2**20, n, dtype=u) << u.type(width - 20)) | rng.integers(0, 4, n, dtype=u)).view(dt)


# ------------------------------------------------------------------------------------------------------------------ boundaries


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundaries(G, dtype):
    """Counts 0, 1, 63, 64, 65, one tile - 1, a tile, a tile + 1, three tiles + 1; k in {1, 2, count / 2, count - 1, count} and 0; both
    directions, sorted or not."""
    rng = np.random.default_rng(171)
    tile = G.plan_top_k(1, 1, dtype)["tile"]
    top = G.TopK()
    for n in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 1):
        keys = random_keys(rng, dtype, n)
        ka = Array(keys)
        for k in sorted({0, 1, 2, n // 2, n - 1, n} & set(range(0, n + 1))):
            for largest in (False, True):
                for sorted_ in (False, True):
                    if n > 65 and k not in (1, n // 2, n) and (largest or sorted_):
                        continue  # (the larger counts: every k smallest and unsorted, three of them in every form)
                    check_case(G, top, keys, k, largest, sorted_, ka=ka)


def test_a_workgroup_walks_more_than_one_tile(G):
    """More tiles than the grid of the streaming kernels has workgroups (8 per CU), uint32: about 8.4 M keys."""
    import torch

    tile = G.plan_top_k(1, 1)["tile"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus * 8 + 3) * tile + 7
    rng = np.random.default_rng(172)
    keys = rng.integers(0, 2**32, n, dtype=np.uint32)
    keys[rng.integers(0, n, 5000)] = keys[17]  # ties, maybe at the threshold
    ka = Array(keys)
    top = G.TopK()
    for k, largest, sorted_ in ((1000, False, True), (n // 8, True, False)):
        last = check_case(G, top, keys, k, largest, sorted_, ka=ka)
        assert last["path"] == CANDIDATES


# ------------------------------------------------------------------------------------------------------------------ ties


@pytest.mark.parametrize("dtype", ["uint32", "float64"])
def test_all_keys_equal(G, dtype):
    n = 3 * G.plan_top_k(1, 1, dtype)["tile"] + 5
    keys = np.full(n, 7.25 if dtype == "float64" else 0xDEADBEEF, dtype=dtype)
    top, ka = G.TopK(), Array(keys)
    for k in (1, 63, n - 1, n):
        for largest in (False, True):
            ok, oi = Array.poisoned(k * keys.dtype.itemsize), Array.poisoned(k * 4)
            top.run_ptr(ka.ptr, n, k, ok.ptr, oi.ptr, key_type=dtype, largest=largest, sorted=True, stream=stream())
            sync()
            assert (oi.result(np.uint32) == np.arange(k)).all()
            assert (ok.result(bits_of(keys).dtype) == bits_of(keys)[0]).all()
            last = top.read_last()
            assert last["ties"] == k and last["path"] == (CANDIDATES if n <= 65536 else FULL)


def test_ties_at_the_threshold(G):
    """Two values with the threshold inside the second; a threshold value whose ties straddle a wave boundary and a tile boundary,
    with need in {1, ties - 1, ties}."""
    rng = np.random.default_rng(173)
    tile = G.plan_top_k(1, 1)["tile"]
    wave = tile // 4
    top = G.TopK()
    n = 2 * tile + 100
    two = np.where(rng.random(n) < 0.3, 5, 9).astype(np.uint32)
    small = int((two == 5).sum())
    for k in (small, small + 1, small + (n - small) // 2, n):
        for sorted_ in (False, True):
            check_case(G, top, two, k, False, sorted_)
            check_case(G, top, two, n - small + 1, True, sorted_)
    # 40 keys below the threshold value scattered about; its ties lie at [wave - 3, wave + 3) and [tile - 2, tile + 4)
    keys = rng.integers(1000, 2**32, n, dtype=np.uint32)
    below = rng.choice(n, 40, replace=False)
    ties = np.concatenate([np.arange(wave - 3, wave + 3), np.arange(tile - 2, tile + 4)])
    below = np.setdiff1d(below, ties)
    keys[below] = rng.integers(0, 500, below.size, dtype=np.uint32)
    keys[ties] = 700
    for need_ in (1, 3, 4, 6, 7, 8, ties.size - 1, ties.size):
        for sorted_ in (False, True):
            last = check_case(G, top, keys, below.size + need_, False, sorted_)
            assert last["ties"] == need_
    inverted = ~keys  # the same picture for the largest
    for need_ in (1, ties.size - 1, ties.size):
        last = check_case(G, top, inverted, below.size + need_, True, False)
        assert last["ties"] == need_


# ------------------------------------------------------------------------------------------------------------------ float order


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_order(G, dtype):
    """-0.0 < +0.0, the infinities, NaNs of both signs beyond them, denormals: the sort's total order on bits, both directions."""
    dt = np.dtype(dtype)
    u = bits_of(np.zeros(1, dtype=dt)).dtype
    sign = u.type(1) << u.type(8 * dt.itemsize - 1)
    tiny = np.finfo(dt).smallest_subnormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny, 1.0, -1.0, np.finfo(dt).max, np.finfo(dt).min, np.finfo(dt).tiny],
                       dtype=dt)
    neg_nan = (bits_of(np.array([np.nan], dtype=dt)) | sign).view(dt)
    payload_nan = (bits_of(np.array([np.nan], dtype=dt)) | u.type(5)).view(dt)
    rng = np.random.default_rng(174)
    keys = np.concatenate([special, neg_nan, payload_nan, rng.choice(special, 2000), rng.standard_normal(300).astype(dt), neg_nan])
    keys = keys[rng.permutation(keys.size)]
    top = G.TopK()
    for k in (1, 2, 7, keys.size // 2, keys.size):
        for largest in (False, True):
            for sorted_ in (False, True):
                check_case(G, top, keys, k, largest, sorted_)
    # the k = 1 answers, said out loud: the smallest is a negative NaN, the largest the positive NaN with the larger payload
    code = key_code(keys, False)
    assert bits_of(keys)[np.argmin(code)] & sign and np.isnan(keys[np.argmin(code)])
    assert bits_of(keys)[np.argmax(code)] == bits_of(payload_nan)[0]


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_signed_integers_with_the_sign_bit_set(G, dtype):
    info = np.iinfo(dtype)
    rng = np.random.default_rng(175)
    keys = np.concatenate([np.array([info.min, info.max, -1, 0, 1, info.min + 1], dtype=dtype),
                           rng.integers(-50, 50, 3000).astype(dtype), rng.integers(info.min, info.max, 3000, dtype=dtype)])
    keys = keys[rng.permutation(keys.size)]
    top = G.TopK()
    for k in (1, 5, 3000, keys.size):
        for largest in (False, True):
            check_case(G, top, keys, k, largest, True)
            check_case(G, top, keys, k, largest, False)
    ok, ka = Array.poisoned(keys.dtype.itemsize), Array(keys)
    top.run_ptr(ka.ptr, keys.size, 1, ok.ptr, key_type=dtype, largest=False, stream=stream())
    sync()
    assert ok.result(dtype)[0] == info.min


# ------------------------------------------------------------------------------------------------------------------ both paths


@pytest.mark.parametrize("dtype", ["uint32", "float32", "uint64", "int64"])
def test_both_paths_at_small_sizes(G, dtype):
    """70001 uniform keys, k = 1000: the threshold's top-digit bucket holds about 34 keys (55 at the most), so CAND_CAPACITY = 64
    takes CANDIDATES and CAND_CAPACITY = 8 takes FULL; a forced CANDIDATES that does not fit reports the fallback and is right."""
    rng = np.random.default_rng(176)
    n, k = 70001, 1000
    u = np.dtype("uint%d" % (8 * np.dtype(dtype).itemsize))
    keys = rng.integers(0, 2**(8 * u.itemsize), n, dtype=u).view(dtype)
    if np.dtype(dtype).kind == "f":
        keys = keys[~np.isnan(keys)]
        n = keys.size
    ka = Array(keys)
    for option, capacity, want in ((AUTO, 64, CANDIDATES), (CANDIDATES, 64, CANDIDATES), (AUTO, 8, FULL), (CANDIDATES, 8, FULL), (FULL, 64, FULL)):
        top = with_options(G, option, capacity)
        for largest in (False, True):
            for sorted_ in (False, True):
                last = check_case(G, top, keys, k, largest, sorted_, ka=ka)
                assert last["path"] == want, (option, capacity, last)
                code = key_code(keys, largest)
                shift = np.uint64(8 * u.itemsize - 11)
                bucket = int(((code >> shift.astype(u)) == (np.sort(code)[k - 1] >> shift.astype(u))).sum())
                assert 8 < bucket <= 64
                assert last["candidates"] == (bucket if want == CANDIDATES else 0)
                plan = G.plan_top_k(n, k, dtype, sorted=sorted_, path=option, cand_capacity=capacity)
                assert last["kernels"] == plan["kernels"]


def test_options_are_checked(G):
    top = G.TopK()
    for name, value in (("PATH", 3), ("PATH", -1), ("CAND_CAPACITY", -1), ("CAND_CAPACITY", 2**30 + 1), ("NOPE", 1)):
        with pytest.raises(G.GluError) as e:
            top.set_option(name, value)
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT and name in e.value.message


# ------------------------------------------------------------------------------------------------------------------ output contract


@pytest.mark.parametrize("dtype", ["uint32", "float64"])
def test_each_output_alone(G, dtype):
    rng = np.random.default_rng(177)
    keys = random_keys(rng, dtype, 20001)
    top = G.TopK()
    both = G.plan_top_k(keys.size, 500, dtype, sorted=True, with_arrays=True)["kernels"]
    for largest in (False, True):
        for sorted_ in (False, True):
            check_case(G, top, keys, 500, largest, sorted_, with_keys=True, with_indices=False, with_kth=False)
            check_case(G, top, keys, 500, largest, sorted_, with_keys=False, with_indices=True, with_kth=False)
            last = check_case(G, top, keys, 500, largest, sorted_, with_keys=False, with_indices=False, with_kth=True)
            assert last["kernels"] == both - 6  # an order statistic: no compaction, no ordering


@pytest.mark.parametrize("dtype,shifts", [("uint32", (4, 8, 12)), ("float32", (4,)), ("uint64", (8,)), ("float64", (8,))])
def test_misaligned_keys(G, dtype, shifts):
    rng = np.random.default_rng(178)
    tile = G.plan_top_k(1, 1, dtype)["tile"]
    top = G.TopK()
    for shift in shifts:
        for n in (tile - 1, tile, 2 * tile + 3):  # (a whole tile behind a shifted base: one tile more than the plan's)
            keys = random_keys(rng, dtype, n)
            check_case(G, top, keys, n // 3, False, True, shift=shift)
            check_case(G, top, keys, n // 3, True, False, shift=shift)
            check_case(G, top, keys, n, True, False, shift=shift)


# ------------------------------------------------------------------------------------------------------------------ refusals


def test_argument_checks_and_overlaps(G):
    import torch

    n = 1000
    keys = np.arange(n, dtype=np.uint32)
    ka, ok, oi, ot = Array(keys), Array.poisoned(4 * n), Array.poisoned(4 * n), Array.poisoned(8)
    top = G.TopK()
    L = G.lib()
    s = stream()

    def refused(text, keys_ptr=ka.ptr, count=n, k=10, out_keys=ok.ptr, out_indices=oi.ptr, out_kth=ot.ptr, key_type=0, handle=None):
        status = L.glu_top_k_run_ptr(top._h if handle is None else handle, keys_ptr, key_type, count, k, 0, 1, out_keys, out_indices, out_kth, s)
        assert status == G.GLU_ERROR_INVALID_ARGUMENT, text
        assert text in L.glu_last_error().decode(), (text, L.glu_last_error())

    refused("top_k is NULL", handle=0)
    refused("Invalid keys buffer", keys_ptr=None)
    refused("Invalid key type", key_type=6)
    refused("Invalid key type", key_type=-1)
    refused("count below 2^32", count=2**32)
    refused("k must not exceed count", k=n + 1)
    refused("k must not exceed count", count=0, k=1, keys_ptr=None)
    refused("all NULL", out_keys=None, out_indices=None, out_kth=None)
    refused("keys is not aligned", keys_ptr=ka.ptr + 2)
    refused("keys is not aligned", keys_ptr=ka.ptr + 4, key_type=3)
    refused("out_keys is not aligned", out_keys=ok.ptr + 1)
    refused("out_keys is not aligned", out_keys=ok.ptr + 4, key_type=5)
    refused("out_indices is not aligned", out_indices=oi.ptr + 2)
    refused("out_kth is not aligned", out_kth=ot.ptr + 2)
    refused("out_kth is not aligned", out_kth=ot.ptr + 4, key_type=4)
    refused("out_keys overlaps keys", out_keys=ka.ptr + 4 * (n - 1))
    refused("out_indices overlaps keys", out_indices=ka.ptr)
    refused("out_kth overlaps keys", out_kth=ka.ptr + 400)
    refused("out_indices overlaps out_keys", out_indices=ok.ptr + 36)
    refused("out_kth overlaps out_keys", out_kth=ok.ptr)
    refused("out_kth overlaps out_indices", out_kth=oi.ptr + 36)
    torch.cuda.synchronize()
    for a in (ok, oi, ot):  # a refused call writes nothing
        assert (a.result(np.uint8) == POISON).all()
    assert (ka.result() == keys).all()
    # arrays that merely touch are fine; k == 0 writes nothing and accepts everything else; count == 0 accepts NULL keys
    top.run_ptr(ka.ptr, n - 10, 10, ka.ptr + 4 * (n - 10), oi.ptr, oi.ptr + 40, stream=s)
    torch.cuda.synchronize()
    assert (ka.result()[n - 10:] == np.arange(10)).all() and (oi.result(np.uint32)[:11] == np.r_[np.arange(10), 9]).all()
    top.run_ptr(None, 0, 0, ok.ptr, None, ot.ptr, stream=s)
    top.run_ptr(ka.ptr, n, 0, ok.ptr, oi.ptr, ot.ptr, stream=s)
    torch.cuda.synchronize()
    assert (ok.result(np.uint8) == POISON).all() and (ot.result(np.uint8) == POISON).all()
    assert top.read_last() == {"path": 0, "candidates": 0, "ties": 0, "kernels": 0}


# ------------------------------------------------------------------------------------------------------------------ capture


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed on
    three contents: uniform keys (CANDIDATES), all keys equal (FULL), few distinct values (FULL); the launch sequence does not depend
    on the data."""
    import torch

    tile = G.plan_top_k(1, 1, "float32")["tile"]
    n, k = 37 * tile + 11, 5000
    rng = np.random.default_rng(179)
    top = G.TopK({"CAND_CAPACITY": 1024})
    kt = torch.empty(n, dtype=torch.float32, device="cuda")
    ok = torch.empty(k + 4, dtype=torch.int32, device="cuda")
    oi = torch.empty(k + 4, dtype=torch.int32, device="cuda")
    ot = torch.empty(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(data):
        kt.copy_(torch.from_numpy(data))
        for t in (ok, oi, ot):
            t.fill_(-1515870811)

    def verify(data, want_path):
        want = expected(data, k, True, True)
        assert (oi.cpu().numpy().view(np.uint32)[:k] == want).all()
        assert (ok.cpu().numpy().view(np.uint32)[:k] == data.view(np.uint32)[want]).all()
        assert (oi.cpu().numpy().view(np.uint32)[k:] == POISON32).all() and (ok.cpu().numpy().view(np.uint32)[k:] == POISON32).all()
        assert ot.cpu().numpy().view(np.uint32)[0] == data.view(np.uint32)[want[-1]]
        assert top.read_last()["path"] == want_path

    def call(s):
        top.run_ptr(kt.data_ptr(), n, k, ok.data_ptr(), oi.data_ptr(), ot.data_ptr(), key_type="float32", largest=True, sorted=True, stream=s)

    # (every bit pattern, NaNs among them: about 74 keys to a top digit, below the capacity of 1024)
    contents = [(rng.integers(0, 2**32, n, dtype=np.uint32).view(np.float32), CANDIDATES), (np.full(n, -2.5, dtype=np.float32), FULL),
                (rng.choice(np.array([1.5, -0.0, 0.0], dtype=np.float32), n), FULL)]
    with torch.cuda.stream(side):
        data, path = contents[0]
        fill(data)
        side.synchronize()
        top.prepare(n, k, "float32")
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(data, path)
        fill(data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(data, path)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for data, path in contents:
            fill(data)
            graph.replay()
            side.synchronize()
            verify(data, path)


def test_the_same_call_gives_the_same_bits_twice(G):
    rng = np.random.default_rng(180)
    keys = (rng.integers(0, 3000, 300001, dtype=np.uint32) * np.uint32(1000003))
    ka = Array(keys)
    top = G.TopK()
    runs = []
    for _ in range(2):
        ok, oi, ot = Array.poisoned(4 * 20000), Array.poisoned(4 * 20000), Array.poisoned(4)
        top.run_ptr(ka.ptr, keys.size, 20000, ok.ptr, oi.ptr, ot.ptr, largest=True, sorted=True, stream=stream())
        sync()
        runs.append((ok.result(np.uint32), oi.result(np.uint32), ot.result(np.uint32), top.read_last()))
    assert all((a == b).all() for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]
    assert (runs[0][1] == expected(keys, 20000, True, True)).all()


# ------------------------------------------------------------------------------------------------------------------ wide indices


def test_indices_past_2_31(G):
    """2^31 + 4097 uint32 keys, a large constant filled on the device, with 300 smaller values planted at known positions on both sides
    of element 2^31; k = 300: the answer is known without a reference."""
    import torch

    from test_gpu_wide_indices import Guarded, need, on_stream, release, small_u32

    n, k = (1 << 31) + 4097, 300
    need(4 * n)
    rng = np.random.default_rng(181)
    pos = np.unique(np.concatenate([[0, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, n - 1], rng.integers(0, 1 << 31, 150),
                                    (1 << 31) + rng.integers(0, 4097, 145)]))
    k = pos.size  # (the number planted; positions on both sides of element 2^31)
    assert (pos < (1 << 31)).sum() > 100 and (pos > (1 << 31)).sum() > 100
    vals = rng.permutation(k).astype(np.int64) * 3 + 1  # distinct, all below the constant
    tile = G.plan_top_k(n, k)["tile"]
    kg = Guarded(4 * n, 4 * tile)
    kv = kg.view(torch.int32)
    kv.fill_(0x7F000000)
    kv[torch.from_numpy(pos.astype(np.int64)).cuda()] = torch.from_numpy(vals.astype(np.int32)).cuda()
    top = G.TopK()
    top.prepare(n, k)
    by_value = np.argsort(vals)
    for sorted_ in (True, False):
        ok, oi, ot = Guarded(4 * k, 4096), Guarded(4 * k, 4096), Guarded(4, 256)
        on_stream(lambda s: top.run_ptr(kg.ptr, n, k, ok.ptr, oi.ptr, ot.ptr, largest=False, sorted=sorted_, stream=s))
        order = by_value if sorted_ else np.argsort(pos)
        assert (small_u32(oi) == pos[order]).all() and (small_u32(ok) == vals[order]).all()
        assert int(small_u32(ot)[0]) == int(vals.max())
        assert ok.intact() and oi.intact() and ot.intact() and kg.intact()
        assert top.read_last()["ties"] == 1
    assert int((kv != 0x7F000000).sum()) == k
    del kg, kv, top
    release()


# ------------------------------------------------------------------------------------------------------------------ with the family


def test_the_top_100_groups_by_sum(G):
    """Sort (key, value) pairs, key runs, a batched reduce (Sum) per run, then the 100 largest sums with their indices, which pick the
    unique keys: against a numpy group-by."""
    import torch

    rng = np.random.default_rng(182)
    n, distinct, max_runs, k = 50021, 900, 1024, 100
    keys = rng.integers(0, distinct, n).astype(np.uint32) * np.uint32(7919)
    vals = rng.integers(0, 1000, n, dtype=np.uint32)
    kt = torch.from_numpy(keys.view(np.int32)).cuda()
    vt = torch.from_numpy(vals.view(np.int32)).cuda()
    offsets, unique, sums, runs_n = (Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4 * max_runs), Array.poisoned(4 * max_runs),
                                     Array.poisoned(4))
    best_sums, best_at = Array.poisoned(4 * k), Array.poisoned(4 * k)
    s = stream()
    G.RadixSort().sort_typed_ptr(kt.data_ptr(), vt.data_ptr(), n, "uint32", s)
    G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum).run_by_key_ptr(G.KeyRuns(), kt.data_ptr(), vt.data_ptr(), sums.ptr, n, offsets.ptr,
                                                                  max_runs, runs_n.ptr, unique.ptr, stream=s)
    # (the entries of sums behind the last run are the sums of empty segments, 0: never among the largest)
    G.TopK().run_ptr(sums.ptr, max_runs, k, best_sums.ptr, best_at.ptr, largest=True, sorted=True, stream=s)
    torch.cuda.synchronize()
    present = np.unique(keys)
    group_sums = np.array([int(vals[keys == key].sum()) for key in present], dtype=np.uint32)
    assert int(runs_n.result(np.uint32)[0]) == present.size
    want = np.argsort(~group_sums, kind="stable")[:k]
    assert (best_at.result(np.uint32) == want).all() and (best_sums.result(np.uint32) == group_sums[want]).all()
    assert (unique.result(np.uint32)[best_at.result(np.uint32)] == present[want]).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_top_k_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
