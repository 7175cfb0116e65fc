"""GPU parity tests of the batched radix sort (glu_radix_sort_run_batch_ptr / glu_radix_sort_run_batch_offsets_ptr): every segment
of an array sorted on its own, stable, ascending, in place.  Expected results come from numpy: the keys are encoded to their
unsigned order here in the test and every segment is ordered by np.argsort(kind="stable") (for very many segments by one
np.lexsort over (encoded key, segment index), which is the same stable order); values are iota, so the stable result is unique."""
import gc
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def encode(keys):
    """The unsigned integers whose order is the sort's order of `keys` (floats: -0 < +0, NaNs beyond the infinities of their sign)."""
    bits = keys.dtype.itemsize * 8
    u = keys.view(np.uint32 if bits == 32 else np.uint64)
    sign = u.dtype.type(1 << (bits - 1))
    if keys.dtype.kind == "u":
        return u
    if keys.dtype.kind == "i":
        return u ^ sign
    return np.where(u & sign, ~u, u | sign)


def expected(keys, vals, offsets):
    offsets = np.asarray(offsets, dtype=np.int64)
    ek, ev = keys.copy(), vals.copy()
    enc = encode(keys)
    if offsets.size - 1 <= 4096:
        for b, e in zip(offsets[:-1], offsets[1:]):
            order = np.argsort(enc[b:e], kind="stable")
            ek[b:e], ev[b:e] = keys[b:e][order], vals[b:e][order]
    else:
        lo, hi = offsets[0], offsets[-1]
        seg = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
        order = np.lexsort((enc[lo:hi], seg))
        ek[lo:hi], ev[lo:hi] = keys[lo:hi][order], vals[lo:hi][order]
    return ek, ev


def to_device(a):
    import torch

    return torch.from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()).cuda()


def same_bits(got, want):
    u = np.uint32 if want.dtype.itemsize == 4 else np.uint64
    return (got.view(u) == want.view(u)).all()


def run_offsets(G, keys, vals, offsets, sorter=None, with_vals=True, prepare=False):
    import torch

    total, nseg = keys.size, len(offsets) - 1
    kt = to_device(keys)
    vt = to_device(vals) if with_vals else None
    ot = to_device(np.asarray(offsets, dtype=np.uint32))
    sorter = sorter or G.RadixSort()
    if prepare:
        sorter.prepare_batch(total, nseg, keys.dtype.itemsize, with_vals)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        sorter.sort_batch_offsets_ptr(kt.data_ptr(), vt.data_ptr() if with_vals else None, total, ot.data_ptr(), nseg, keys.dtype.name,
                                      st.cuda_stream)
        st.synchronize()
        gk = kt.cpu().numpy().view(keys.dtype)
        gv = vt.cpu().numpy().view(np.uint32) if with_vals else None
    return gk, gv, sorter


def check_offsets(G, keys, offsets, with_vals=True, **kw):
    vals = np.arange(keys.size, dtype=np.uint32)
    gk, gv, sorter = run_offsets(G, keys, vals, offsets, with_vals=with_vals, **kw)
    ek, ev = expected(keys, vals, offsets)
    assert same_bits(gk, ek), "keys differ"
    if with_vals:
        assert (gv == ev).all(), "values differ (stability)"
    return sorter


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


def mixed_lengths(rng, tiny, small, medium, large):
    """Zeros, ones, geometric around 40, uniform up to 3000 and the given long ones, shuffled."""
    lens = np.concatenate([np.zeros(tiny, np.int64), np.ones(tiny, np.int64), rng.geometric(1 / 40.0, small),
                           rng.integers(0, 3001, medium), np.asarray(large, dtype=np.int64)])
    rng.shuffle(lens)
    return lens


def random_keys(rng, n, name):
    if name in ("float32", "float64"):
        k = rng.standard_normal(n).astype(name)
        u = np.uint32 if name == "float32" else np.uint64
        nan = np.array([np.nan], dtype=name).view(u)[0]
        sign = u(1 << (k.dtype.itemsize * 8 - 1))
        special = np.array([0.0, -0.0, np.inf, -np.inf], dtype=name).view(u)
        special = np.concatenate([special, [nan, nan | sign, nan | u(1), nan | sign | u(5)]]).astype(u)
        where = rng.choice(n, size=min(n, max(8, n // 50)), replace=False)
        k.view(u)[where] = special[rng.integers(0, special.size, where.size)]
        return k
    info = np.iinfo(name)
    return rng.integers(info.min, int(info.max) + 1, n, dtype=name)


@pytest.mark.parametrize("num_partitions", [1, 3, 1000])
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 500, 513, 1000, 4096, 5000, 16384])
def test_equal_partitions(G, count, num_partitions):
    import torch

    num_partitions = min(num_partitions, (1 << 22) // count)
    rng = np.random.default_rng(count * 7 + num_partitions)
    n = count * num_partitions
    keys = rng.integers(0, 2**32, n, dtype=np.uint32)
    keys[::5] &= np.uint32(0xFF0000FF)
    vals = np.arange(n, dtype=np.uint32)
    kt, vt = to_device(keys), to_device(vals)
    sorter = G.RadixSort()
    sorter.sort_batch_ptr(kt.data_ptr(), vt.data_ptr(), count, num_partitions, "uint32", torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ek, ev = expected(keys, vals, np.arange(num_partitions + 1) * count)
    assert (kt.cpu().numpy().view(np.uint32) == ek).all() and (vt.cpu().numpy().view(np.uint32) == ev).all()
    path = G.plan_batch(count)[0]
    rb = sorter.read_batch()
    assert [rb["wave"], rb["block"], rb["long"]] == [num_partitions if path == p else 0 for p in (1, 2, 3)]


def test_equal_partitions_longer_than_a_tile(G):
    """20000 x 5: the looped path (every partition is sorted by the ordinary sort)."""
    import torch

    count, num_partitions = 20000, 5
    rng = np.random.default_rng(20000)
    keys = rng.integers(0, 2**32, count * num_partitions, dtype=np.uint32)
    vals = np.arange(keys.size, dtype=np.uint32)
    kt, vt = to_device(keys), to_device(vals)
    sorter = G.RadixSort()
    sorter.sort_batch_ptr(kt.data_ptr(), vt.data_ptr(), count, num_partitions, "uint32", torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ek, ev = expected(keys, vals, np.arange(num_partitions + 1) * count)
    assert (kt.cpu().numpy().view(np.uint32) == ek).all() and (vt.cpu().numpy().view(np.uint32) == ev).all()
    assert sorter.read_batch() == {"wave": 0, "block": 0, "long": 5}


@pytest.mark.parametrize("with_vals", [True, False])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_every_key_type_on_mixed_lengths(G, key_type, with_vals):
    rng = np.random.default_rng(KEY_TYPES.index(key_type) + 10 * with_vals)
    lens = mixed_lengths(rng, 50, 600, 120, [513, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 40000])
    offsets = offsets_of(lens)
    keys = random_keys(rng, int(offsets[-1]), key_type)
    sorter = check_offsets(G, keys, offsets, with_vals=with_vals)
    rb = sorter.read_batch()
    assert rb["wave"] > 0 and rb["block"] > 0 and rb["long"] > 0
    assert rb["wave"] + rb["block"] + rb["long"] == int((lens >= 2).sum())


def test_every_class_in_one_call(G):
    """About 4 M pairs whose segment lengths hit the three classes in ONE call; read_batch must account for every segment."""
    rng = np.random.default_rng(4)
    lens = mixed_lengths(rng, 3000, 20000, 800, [16384, 16384, 16385, 16385, 100000, 100000, 100001, 1500000])
    offsets = offsets_of(lens)
    total = int(offsets[-1])
    assert 3_500_000 < total < 5_000_000
    keys = rng.integers(0, 2**32, total, dtype=np.uint32)
    sorter = check_offsets(G, keys, offsets)
    rb = sorter.read_batch()
    assert rb["wave"] > 0 and rb["block"] > 0 and rb["long"] > 0
    assert rb["long"] == int((lens > 16384).sum())
    assert rb["wave"] + rb["block"] + rb["long"] + int((lens == 0).sum()) + int((lens == 1).sum()) == lens.size


@pytest.mark.parametrize("kind", ["ten_values", "all_equal"])
def test_duplicate_heavy_keys_stay_in_input_order(G, kind):
    rng = np.random.default_rng(11)
    lens = mixed_lengths(rng, 20, 2000, 200, [5000, 16384, 30000, 200000])
    offsets = offsets_of(lens)
    total = int(offsets[-1])
    keys = rng.integers(0, 10, total, dtype=np.uint32) if kind == "ten_values" else np.full(total, 0xDEADBEEF, dtype=np.uint32)
    check_offsets(G, keys, offsets)


def test_elements_outside_the_segments_are_not_touched(G):
    rng = np.random.default_rng(12)
    lens = mixed_lengths(rng, 10, 500, 50, [9000, 20000])
    head, tail = 777, 1234
    offsets = offsets_of(lens) + head
    total = int(offsets[-1]) + tail
    keys = rng.integers(0, 2**32, total, dtype=np.uint32)
    keys[:head] = np.arange(head, 0, -1, dtype=np.uint32) + np.uint32(0xF0000000)  # descending sentinels: any sort would move them
    keys[total - tail:] = np.arange(tail, 0, -1, dtype=np.uint32)
    vals = np.arange(total, dtype=np.uint32)
    gk, gv, _ = run_offsets(G, keys, vals, offsets)
    assert (gk[:head] == keys[:head]).all() and (gv[:head] == vals[:head]).all()
    assert (gk[total - tail:] == keys[total - tail:]).all() and (gv[total - tail:] == vals[total - tail:]).all()
    ek, ev = expected(keys, vals, offsets)
    assert (gk == ek).all() and (gv == ev).all()


def test_a_million_tiny_segments(G):
    """2^20 segments of 0 .. 8 elements: binning and list walking at scale."""
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 9, 1 << 20)
    offsets = offsets_of(lens)
    keys = rng.integers(0, 2**32, int(offsets[-1]), dtype=np.uint32)
    sorter = check_offsets(G, keys, offsets)
    rb = sorter.read_batch()
    assert rb == {"wave": int((lens >= 2).sum()), "block": 0, "long": 0}


def test_prepared_batch_allocates_nothing_and_replays_from_a_graph(G):
    """After prepare_batch the call leaves scratch_size() alone; captured into a graph it is replayed on new data in the same
    buffers and on DIFFERENT offsets in the same offsets array (the segments are binned on the device in every replay)."""
    import torch

    rng = np.random.default_rng(14)
    total, nseg = 1_200_000, 3000

    def draw_offsets():
        lens = mixed_lengths(rng, 200, 2000, 590, [700, 5000, 9000, 16384, 17000, 60000, 0, 0, 0, 0])
        assert lens.size == nseg
        return np.minimum(offsets_of(lens), total)

    sorter = G.RadixSort()
    sorter.prepare_batch(total, nseg, 4, True)
    size = sorter.scratch_size()
    assert size > 0
    kt = torch.empty(total, dtype=torch.int32, device="cuda")
    vt = torch.empty(total, dtype=torch.int32, device="cuda")
    ot = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(keys, vals, offsets):
        kt.copy_(torch.from_numpy(keys.view(np.int32)))
        vt.copy_(torch.from_numpy(vals.view(np.int32)))
        ot.copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))

    with torch.cuda.stream(side):
        keys, vals, offsets = rng.integers(0, 2**32, total, dtype=np.uint32), np.arange(total, dtype=np.uint32), draw_offsets()
        fill(keys, vals, offsets)
        sorter.sort_batch_offsets_ptr(kt.data_ptr(), vt.data_ptr(), total, ot.data_ptr(), nseg, "uint32", side.cuda_stream)  # warm-up
        side.synchronize()
        assert sorter.scratch_size() == size
        ek, ev = expected(keys, vals, offsets)
        assert (kt.cpu().numpy().view(np.uint32) == ek).all() and (vt.cpu().numpy().view(np.uint32) == ev).all()
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            sorter.sort_batch_offsets_ptr(kt.data_ptr(), vt.data_ptr(), total, ot.data_ptr(), nseg, "uint32",
                                          torch.cuda.current_stream().cuda_stream)
        assert sorter.scratch_size() == size
        for rep in range(3):
            keys = rng.integers(0, 2**32 if rep else 50, total, dtype=np.uint32)
            offsets = draw_offsets()
            fill(keys, vals, offsets)
            graph.replay()
            side.synchronize()
            ek, ev = expected(keys, vals, offsets)
            assert (kt.cpu().numpy().view(np.uint32) == ek).all() and (vt.cpu().numpy().view(np.uint32) == ev).all()
            rb = sorter.read_batch()
            lens = np.diff(offsets)
            assert rb["wave"] + rb["block"] + rb["long"] == int((lens >= 2).sum())


def test_two_objects_on_two_streams_concurrently(G):
    import torch

    rng = np.random.default_rng(15)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sorters = [G.RadixSort(), G.RadixSort()]
    jobs = []
    for i in range(2):
        lens = mixed_lengths(rng, 100, 5000 + 3000 * i, 300, [16384, 20000 + i, 300000])
        offsets = offsets_of(lens)
        keys = rng.integers(0, 2**32, int(offsets[-1]), dtype=np.uint32)
        vals = np.arange(keys.size, dtype=np.uint32)
        jobs.append((keys, vals, offsets, to_device(keys), to_device(vals), to_device(offsets.astype(np.uint32))))
        sorters[i].prepare_batch(keys.size, lens.size, 4, True)
    torch.cuda.synchronize()
    for rep in range(2):
        for i in (0, 1):
            keys, vals, offsets, kt, vt, ot = jobs[i]
            with torch.cuda.stream(streams[i]):
                if rep:
                    kt.copy_(torch.from_numpy(keys.view(np.int32)))
                    vt.copy_(torch.from_numpy(vals.view(np.int32)))
                sorters[i].sort_batch_offsets_ptr(kt.data_ptr(), vt.data_ptr(), keys.size, ot.data_ptr(), offsets.size - 1, "uint32",
                                                  streams[i].cuda_stream)
        for st in streams:
            st.synchronize()
        for keys, vals, offsets, kt, vt, ot in jobs:
            ek, ev = expected(keys, vals, offsets)
            assert (kt.cpu().numpy().view(np.uint32) == ek).all() and (vt.cpu().numpy().view(np.uint32) == ev).all()


MALFORMED_TOTAL = 40000
MALFORMED_GUARD = 512  # elements of poison in front of and behind the arrays; every malformed entry exceeds `total` by less
MALFORMED_OFFSETS = {
    # every segment ends below its begin
    "descending": [MALFORMED_TOTAL, 30000, 20000, 5000, 300, 0],
    # every segment ends beyond total, or begins there and ends below its begin
    "beyond_total": [0, MALFORMED_TOTAL + 1, MALFORMED_TOTAL + 300, 5, MALFORMED_TOTAL + 5, 100, MALFORMED_TOTAL + 511],
    # well-formed segments of every class, pairwise disjoint, in front of and among malformed ones
    "mixed": [0, 300, 900, 5900, 26000, 30000, MALFORMED_TOTAL + 50, 35000, 36000, MALFORMED_TOTAL + 511, 31000, 31000, 32000,
              MALFORMED_TOTAL + 1],
}


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
@pytest.mark.parametrize("case", ["descending", "beyond_total", "mixed"])
def test_malformed_offsets_touch_nothing_outside_the_array(G, case, key_type):
    """A segment whose end is below its begin or beyond `total` is empty to every kernel: the call returns GLU_OK, the poison in front
    of and behind the keys and the values is intact (a kernel that trusted an end up to 511 elements beyond `total` would sort poison
    into the array), [0, total) is a permutation of what it held with every value still beside its key, and every well-formed segment
    that overlaps no malformed one (taken by its span between begin and end, cut at total) is sorted exactly."""
    import torch

    total, guard, offsets = MALFORMED_TOTAL, MALFORMED_GUARD, MALFORMED_OFFSETS[case]
    assert max(offsets) < total + guard
    rng = np.random.default_rng(600 + len(case))
    u = np.dtype(key_type)
    keys = rng.integers(0, 2 ** (8 * u.itemsize), total, dtype=u)
    keys[::3] &= u.type(0xFFFF)  # ties: the values tell a stable sort from another one
    vals = np.arange(total, dtype=np.uint32)
    poison_k, poison_v = np.full(guard, 0xA5A5A5A5A5A5A5A5 >> (64 - 8 * u.itemsize), dtype=u), np.full(guard, 0xA5A5A5A5, dtype=np.uint32)
    kt, vt = to_device(np.concatenate([poison_k, keys, poison_k])), to_device(np.concatenate([poison_v, vals, poison_v]))
    ot = to_device(np.asarray(offsets, dtype=np.uint32))
    sorter = G.RadixSort()
    sorter.sort_batch_offsets_ptr(kt.data_ptr() + guard * u.itemsize, vt.data_ptr() + guard * 4, total, ot.data_ptr(), len(offsets) - 1, key_type,
                                  torch.cuda.current_stream().cuda_stream)  # (GluError if the status is not GLU_OK)
    torch.cuda.synchronize()
    gk, gv = kt.cpu().numpy().view(u), vt.cpu().numpy().view(np.uint32)
    assert (gk[:guard] == poison_k).all() and (gk[guard + total:] == poison_k).all(), "the call wrote keys outside the array"
    assert (gv[:guard] == poison_v).all() and (gv[guard + total:] == poison_v).all(), "the call wrote values outside the array"
    assert (ot.cpu().numpy().view(np.uint32) == np.asarray(offsets, dtype=np.uint32)).all(), "the call wrote to the offsets"
    gk, gv = gk[guard:guard + total], gv[guard:guard + total]
    assert (np.sort(gv) == vals).all(), "[0, total) is no permutation of what it held"
    assert (gk == keys[gv]).all(), "a value left its key"
    pairs = list(zip(offsets[:-1], offsets[1:]))
    malformed = [(min(b, e), min(max(b, e), total)) for b, e in pairs if e < b or e > total]
    clear = [(b, e) for b, e in pairs if b <= e <= total and not any(lo < e and b < hi for lo, hi in malformed)]
    assert case != "mixed" or {G.plan_batch(e - b, u.itemsize)[0] for b, e in clear} == {1, 2, 3}, "the clear segments miss a class"
    ek, ev = keys.copy(), vals.copy()
    for b, e in clear:
        order = np.argsort(keys[b:e], kind="stable")
        ek[b:e], ev[b:e] = keys[b:e][order], vals[b:e][order]
        assert (gk[b:e] == ek[b:e]).all() and (gv[b:e] == ev[b:e]).all(), (case, key_type, b, e)
    rb = sorter.read_batch()
    assert rb["wave"] + rb["block"] + rb["long"] <= sum(1 for b, e in pairs if b < e <= total)


def test_argument_checks(G):
    import torch

    sorter = G.RadixSort()
    kt = torch.zeros(64, dtype=torch.int64, device="cuda")
    ot = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad = [
        lambda: sorter.sort_batch_ptr(None, None, 8, 8),                                # NULL keys with a non-zero size
        lambda: sorter.sort_batch_ptr(kt.data_ptr(), None, 1 << 20, 1 << 12),           # count * num_partitions = 2^32
        lambda: sorter.sort_batch_ptr(kt.data_ptr() + 4, None, 8, 4, "uint64"),         # misaligned 8-byte keys
        lambda: sorter.sort_batch_ptr(kt.data_ptr(), kt.data_ptr() + 2, 8, 4),          # misaligned values
        lambda: sorter.sort_batch_offsets_ptr(kt.data_ptr(), None, 64, None, 3),        # NULL offsets
        lambda: sorter.sort_batch_offsets_ptr(kt.data_ptr(), None, 64, ot.data_ptr() + 2, 3),
        lambda: lib_call_with_key_type(G, sorter, kt, 9),                               # unknown key type
    ]
    for call in bad:
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT
    sorter.sort_batch_ptr(None, None, 0, 5)  # nothing to sort: NULL arrays are fine
    sorter.sort_batch_offsets_ptr(None, None, 0, ot.data_ptr(), 3)


def lib_call_with_key_type(G, sorter, kt, key_type):
    import ctypes

    G.check(G.lib().glu_radix_sort_run_batch_ptr(sorter._h, ctypes.c_void_p(kt.data_ptr()), None, 8, 4, key_type, None))


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_batch_sort_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
