"""GPU tests of batched top-k (glu_top_k_run_batch_ptr, glu_top_k_run_batch_offsets_ptr): the k best keys of every segment, every
array bit for bit against numpy.argsort(code(segment), kind="stable")[:min(k, len)] per segment, where code is the sort's key code
(complemented for largest); indices local to the segment, rows of stride k, untouched entries still poison.  The class limits, the
loop threshold and the kernel counts are read from glu_top_k_plan_batch, never written here."""
import gc
import os
import subprocess

import numpy as np
import pytest

from test_gpu_top_k import POISON, POISON32, Array, bits_of, random_keys, stream, sync
from test_top_k_pick import DTYPES, key_code

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = ((False, True), (True, True), (False, False), (True, False))  # (largest, sorted)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def poison_of(u):
    return np.frombuffer(bytes([POISON]) * np.dtype(u).itemsize, dtype=u)[0]


def clamp_segments(offsets, total):
    """[(begin, len)]: a segment that ends below its begin or beyond total is empty (batch_offsets_segment)."""
    out = []
    for b, e in zip(offsets[:-1], offsets[1:]):
        b, e = int(b), int(e)
        out.append((b, 0 if e < b or e > total else e - b))
    return out


def expected(keys, segs, k, largest, sorted_):
    """out_keys, out_indices, out_kth as the contract leaves poisoned arrays."""
    u = bits_of(keys).dtype
    bits = bits_of(keys)
    ek, ei, et = np.full(len(segs) * k, poison_of(u), dtype=u), np.full(len(segs) * k, POISON32, dtype=np.uint32), np.full(len(segs), poison_of(u), dtype=u)
    for s, (b, n) in enumerate(segs):
        if n == 0 or k == 0:
            continue
        ks = min(k, n)
        head = np.argsort(key_code(keys[b:b + n], largest), kind="stable")[:ks]
        et[s] = bits[b + head[-1]]
        if not sorted_:
            head = np.sort(head)
        ek[s * k:s * k + ks] = bits[b + head]
        ei[s * k:s * k + ks] = head
    return ek, ei, et


def run_case(G, top, keys, k, largest=False, sorted_=True, offsets=None, count=None, parts=None, shift=0, with_keys=True, with_indices=True,
             with_kth=True, ka=None, loop_min=0, case=None):
    """One batched call and everything the contract says of it; returns read_batch()."""
    kb, name, u = keys.dtype.itemsize, keys.dtype.name, bits_of(keys).dtype
    ka = ka or Array(keys, shift)
    if offsets is not None:
        nseg, segs = len(offsets) - 1, clamp_segments(offsets, keys.size)
        oa = Array(np.asarray(offsets, dtype=np.uint32))
    else:
        nseg, segs = parts, [(s * count, count) for s in range(parts)]
    ok, oi, ot = Array.poisoned((nseg * k + 5) * kb), Array.poisoned((nseg * k + 5) * 4), Array.poisoned((nseg + 3) * kb)
    outs = (ok.ptr if with_keys else None, oi.ptr if with_indices else None, ot.ptr if with_kth else None)
    if offsets is not None:
        top.run_batch_offsets_ptr(ka.ptr, keys.size, oa.ptr, nseg, k, *outs, key_type=name, largest=largest, sorted=sorted_, stream=stream())
    else:
        top.run_batch_ptr(ka.ptr, count, parts, k, *outs, key_type=name, largest=largest, sorted=sorted_, stream=stream())
    sync()
    case = (case, name, k, largest, sorted_, shift, keys.size, nseg)
    ek, ei, et = expected(keys, segs, k, largest, sorted_)
    got_k, got_i, got_t = ok.result(u), oi.result(np.uint32), ot.result(u)
    assert (got_k[:nseg * k] == (ek if with_keys else poison_of(u))).all(), case
    assert (got_i[:nseg * k] == (ei if with_indices else POISON32)).all(), case
    assert (got_t[:nseg] == (et if with_kth else poison_of(u))).all(), case
    assert (got_k[nseg * k:] == poison_of(u)).all() and (got_i[nseg * k:] == POISON32).all() and (got_t[nseg:] == poison_of(u)).all(), case
    assert (ka.result(u) == bits_of(keys)).all(), "batched top-k wrote to its input"
    if offsets is not None:
        assert (oa.result(np.uint32) == np.asarray(offsets, dtype=np.uint32)).all(), "batched top-k wrote to the offsets"
    last = top.read_batch()
    plan = G.plan_top_k_batch(keys.size if offsets is not None else count, nseg, k, name, offsets_form=offsets is not None, sorted=sorted_,
                              with_arrays=with_keys or with_indices, loop_min=loop_min)
    assert last["kernels"] == plan["kernels"], (case, last, plan)
    return last, plan


def classes_of(G, segs, dtype):
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    want = {"wave": 0, "block": 0, "long": 0}
    for _, n in segs:
        if n:
            want["wave" if n <= limits[0] else "block" if n <= limits[3] else "long"] += 1
    return want


def boundary_lengths(G, dtype):
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    assert limits == sorted(limits) and limits[0] == 512
    out = [0, 1, 2, 63, 64, 65, 511, 512, 513]
    for limit in limits:
        out += [limit - 1, limit, limit + 1]
    return sorted(set(out + [3 * limits[3] + 17])), limits


def offsets_of(lengths, first):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ boundaries


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundaries_with_offsets(G, dtype):
    """Every boundary length as a segment of one batch that starts at an odd element; k from 1 to beyond the longest segment (rows end
    in poison behind k_s); both directions, sorted or not; the keys 0, 4 and 8 bytes behind a 16-byte boundary."""
    rng = np.random.default_rng(181)
    lengths, limits = boundary_lengths(G, dtype)
    lengths = [lengths[i] for i in rng.permutation(len(lengths))] + [0, 3]
    offsets = offsets_of(lengths, 3)
    keys = random_keys(rng, dtype, int(offsets[-1]) + 5)
    top = G.TopK()
    ks = [1, 2, 32, 64, 511, 513, limits[1] // 2, limits[3], 3 * limits[3] + 16, 3 * limits[3] + 20]
    for shift in (0, 4, 8):
        if shift % keys.dtype.itemsize:
            continue
        ka = Array(keys, shift)
        for i, k in enumerate(ks):
            for largest, sorted_ in (COMBOS if shift == 0 and k in (2, 513, limits[3]) else (COMBOS[(i + shift // 4) % 4],)):
                last, _ = run_case(G, top, keys, k, largest, sorted_, offsets=offsets, shift=shift, ka=ka)
                assert {c: last[c] for c in ("wave", "block", "long")} == classes_of(G, clamp_segments(offsets, keys.size), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundaries_with_equal_partitions(G, dtype):
    """Three partitions of every boundary length; k in {1, 2, len / 2, len - 1, len}."""
    rng = np.random.default_rng(182)
    lengths, _ = boundary_lengths(G, dtype)
    top = G.TopK()
    i = 0
    for n in lengths:
        keys = random_keys(rng, dtype, 3 * n)
        shift = (0, 8, 4)[i % 3] if keys.dtype.itemsize == 4 else (0, 8)[i % 2]
        ka = Array(keys, shift)
        for k in sorted({0, 1, 2, n // 2, n - 1, n} & set(range(0, n + 1))):
            largest, sorted_ = COMBOS[i % 4]
            i += 1
            last, plan = run_case(G, top, keys, k, largest, sorted_, count=n, parts=3, shift=shift, ka=ka)
            want = {"wave": 0, "block": 0, "long": 0}
            if plan["path"] != G.TopKBatch_None:
                want[{G.TopKBatch_Wave: "wave", G.TopKBatch_Block: "block", G.TopKBatch_Long: "long"}[plan["path"]]] = 3
            assert {c: last[c] for c in want} == want and (plan["path"] == G.TopKBatch_None) == (n == 0 or k == 0)


# ------------------------------------------------------------------------------------------------------------------ one mixed batch


def mixed_lengths(rng, limits, nseg):
    pick = rng.integers(0, 100, nseg)
    lengths = np.where(pick < 15, 0, np.where(pick < 70, rng.integers(1, limits[0] + 1, nseg), np.where(pick < 90, rng.integers(limits[0] + 1, limits[1] + 1, nseg),
                       np.where(pick < 96, rng.integers(limits[1] + 1, limits[2] + 1, nseg), rng.integers(limits[2] + 1, limits[3] + 1, nseg)))))
    lengths[rng.integers(0, nseg, 3)] = limits[3] + rng.integers(1, 4000, 3)
    return lengths


@pytest.mark.parametrize("dtype,largest,sorted_", [("uint32", False, True), ("float32", True, False), ("int64", True, True)])
def test_one_mixed_batch(G, dtype, largest, sorted_):
    rng = np.random.default_rng(183)
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    offsets = offsets_of(mixed_lengths(rng, limits, 2000), 1)
    keys = random_keys(rng, dtype, int(offsets[-1]))
    last, _ = run_case(G, G.TopK(), keys, 40, largest, sorted_, offsets=offsets)
    want = classes_of(G, clamp_segments(offsets, keys.size), dtype)
    assert min(want.values()) > 0 and {c: last[c] for c in want} == want


# ------------------------------------------------------------------------------------------------------------------ ties and floats


@pytest.mark.parametrize("dtype", ("uint32", "float64"))
def test_ties(G, dtype):
    """All keys equal; two values; a threshold value with more ties than needed that straddle a wave boundary of the wave class (a
    lane boundary too), a tile boundary of the compaction and the end of a pack."""
    rng = np.random.default_rng(184)
    dt = np.dtype(dtype)
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    lengths = [300, 512, limits[1], limits[3], 2 * limits[3] + 5]
    offsets = offsets_of(lengths, 1)
    total = int(offsets[-1])
    top = G.TopK()
    u = bits_of(np.zeros(1, dt)).dtype
    for kind in ("equal", "two", "straddle"):
        if kind == "equal":
            keys = np.full(total, 0x3F8C0FFE, dtype=u).view(dt)
        elif kind == "two":
            keys = rng.choice(np.array([7, 0x40000001], dtype=u), total).view(dt)
        else:
            keys = np.full(total, 0x50000000, dtype=u)
            for b, n in clamp_segments(offsets, total):
                low = rng.choice(n, min(n // 3, 90), replace=False)
                keys[b + low] = rng.integers(0, 1000, low.size)  # below the threshold value 0x50000000, of which there are more than needed
            keys = keys.view(dt)
        for k in (1, 64, 100, 257, 4097):
            for largest, sorted_ in COMBOS[:2] if k != 100 else COMBOS:
                run_case(G, top, keys, k, largest, sorted_, offsets=offsets, case=kind)


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_float_order(G, dtype):
    """NaNs of both signs, +-0 and +-inf among the keys: the order is the sort's order on bits."""
    rng = np.random.default_rng(185)
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    lengths = [9, 200, limits[1] + 1, limits[3] + 9]
    offsets = offsets_of(lengths, 1)
    special = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], dtype=dtype)
    special[1] = -special[0]
    keys = np.where(rng.integers(0, 3, int(offsets[-1])) == 0, rng.standard_normal(int(offsets[-1])).astype(dtype), rng.choice(special, int(offsets[-1])))
    keys = keys.astype(dtype)
    top = G.TopK()
    for k in (1, 5, 150):
        for largest, sorted_ in COMBOS:
            run_case(G, top, keys, k, largest, sorted_, offsets=offsets)


# ------------------------------------------------------------------------------------------------------------------ the output contract


def test_every_subset_of_the_outputs(G):
    rng = np.random.default_rng(186)
    limits = G.plan_top_k_batch(1, 1, 1, "int32")["limits"]
    offsets = offsets_of([0, 100, limits[1], 0, limits[3] + 100, 7], 1)
    keys = random_keys(rng, "int32", int(offsets[-1]))
    top = G.TopK()
    for mask in range(1, 8):
        for sorted_ in (True, False):
            run_case(G, top, keys, 9, True, sorted_, offsets=offsets, with_keys=bool(mask & 1), with_indices=bool(mask & 2), with_kth=bool(mask & 4))
            run_case(G, top, keys[:6 * 700], 9, False, sorted_, count=700, parts=6, with_keys=bool(mask & 1), with_indices=bool(mask & 2),
                     with_kth=bool(mask & 4))


def test_nothing_to_do_writes_nothing(G):
    rng = np.random.default_rng(187)
    keys = random_keys(rng, "uint32", 1000)
    top = G.TopK()
    offsets = offsets_of([100] * 10, 0)
    for k, kwargs in ((0, dict(offsets=offsets)), (0, dict(count=100, parts=10)), (4, dict(offsets=offsets[:1])), (4, dict(count=100, parts=0)),
                      (0, dict(count=0, parts=7))):
        last, plan = run_case(G, top, keys, k, **kwargs)
        assert plan["path"] == G.TopKBatch_None and last == {"wave": 0, "block": 0, "long": 0, "kernels": 0}


def test_malformed_offsets(G):
    """Decreasing offsets and ends beyond total: those segments' rows stay untouched, the others are right, the guards intact."""
    rng = np.random.default_rng(188)
    limits = G.plan_top_k_batch(1, 1, 1, "uint32")["limits"]
    total = 3 * limits[3]
    keys = random_keys(rng, "uint32", total)
    offsets = np.array([5, 300, 200, 1000, total + 1, 2**32 - 1, 40, 40 + limits[2], total, 0, limits[3] + 77, 2**31, 9], dtype=np.int64)
    assert sum(n > 0 for _, n in clamp_segments(offsets, total)) >= 4
    top = G.TopK()
    for largest, sorted_ in COMBOS:
        run_case(G, top, keys, 50, largest, sorted_, offsets=offsets)


# ------------------------------------------------------------------------------------------------------------------ loop, sorted stage


@pytest.mark.parametrize("dtype", ("uint32", "float64"))
def test_loop_path_gives_the_long_kernels_bits(G, dtype):
    """Equal partitions on both sides of BATCH_LOOP_MIN, set small: the single call partition after partition and the class kernels
    are held against the same expectation, so their bits are identical."""
    rng = np.random.default_rng(189)
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    n = limits[3] + 1000
    keys = random_keys(rng, dtype, 4 * n)
    ka = Array(keys)
    for loop_min, path in ((n, G.TopKBatch_Loop), (n + 1, G.TopKBatch_Long)):
        top = G.TopK({"BATCH_LOOP_MIN": loop_min})
        for largest, sorted_ in COMBOS:
            last, plan = run_case(G, top, keys, 77, largest, sorted_, count=n, parts=4, ka=ka, loop_min=loop_min)
            assert plan["path"] == path and plan["loop_min"] == loop_min and last["long"] == 4
        run_case(G, top, keys, 77, False, False, count=n, parts=4, ka=ka, loop_min=loop_min, with_keys=False, with_indices=False)


@pytest.mark.parametrize("dtype", ("uint32", "int64"))
def test_sorted_stage_around_the_batched_sorts_limits(G, dtype):
    """k on both sides of the batched sort's wave limit and of its single-block limit (beyond it the stage is one sort per row, and
    the plan counts it so)."""
    rng = np.random.default_rng(190)
    kb = np.dtype(dtype).itemsize
    ks = set()
    for n in (2, 100000):  # the wave class's tile and the largest workgroup tile of the batched sort
        path, tile = G.plan_batch(n, kb)
        ks |= {tile, tile + 1}
    assert G.plan_batch(max(ks) - 1, kb)[0] == 2 and G.plan_batch(max(ks), kb)[0] == 3
    top = G.TopK()
    for k in sorted(ks):
        lengths = [k + 10, k // 2, k, 2 * k + 1, 0]
        offsets = offsets_of(lengths, 1)
        keys = random_keys(rng, dtype, int(offsets[-1]))
        for largest in (False, True):
            run_case(G, top, keys, k, largest, True, offsets=offsets)
    singly = G.plan_top_k_batch(1 << 20, 8, 1 << 17, dtype)["kernels"]
    assert singly == G.plan_top_k_batch(1 << 20, 8, 1 << 17, dtype, sorted=False)["kernels"] + 8 + 1


# ------------------------------------------------------------------------------------------------------------------ determinism, capture, composition


def test_capture_replays_on_new_contents_and_twice_gives_the_same_bits(G):
    import torch

    rng = np.random.default_rng(191)
    limits = G.plan_top_k_batch(1, 1, 1, "float32")["limits"]
    lengths = mixed_lengths(rng, limits, 300)
    offsets = offsets_of(lengths, 0)
    total, nseg, k = int(offsets[-1]), 300, 17
    segs = clamp_segments(offsets, total)
    top = G.TopK()
    top.prepare_batch(total, nseg, k, "float32")
    d_keys = torch.zeros(total, dtype=torch.float32, device="cuda")
    d_off = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    ok, oi, ot = (torch.zeros(nseg * k, dtype=torch.int32, device="cuda") for _ in range(3))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def call(s):
        top.run_batch_offsets_ptr(d_keys.data_ptr(), total, d_off.data_ptr(), nseg, k, ok.data_ptr(), oi.data_ptr(), ot.data_ptr(),
                                  key_type="float32", largest=True, sorted=True, stream=s)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # (fills, replays and read-backs all on the stream of the capture)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        seen = []
        for round_ in range(3):
            keys = random_keys(np.random.default_rng(500 + round_ // 2), "float32", total)  # (rounds 0 and 1: the same contents)
            d_keys.copy_(torch.from_numpy(keys.view(np.int32)).view(torch.float32))
            ok.fill_(-1), oi.fill_(-1), ot.fill_(-1)
            graph.replay()
            side.synchronize()
            ek, ei, et = expected(keys, segs, k, True, True)
            got = (ok.cpu().numpy().view(np.uint32), oi.cpu().numpy().view(np.uint32), ot.cpu().numpy().view(np.uint32)[:nseg])
            mask = (np.arange(k)[None, :] < np.minimum(lengths, k)[:, None]).ravel()
            assert (got[0][mask] == ek[mask]).all() and (got[1][mask] == ei[mask]).all() and (got[0][~mask] == 0xFFFFFFFF).all()
            assert (got[2][lengths > 0] == et[lengths > 0]).all() and (got[2][lengths == 0] == 0xFFFFFFFF).all()
            seen.append(got)
    assert all((a == b).all() for a, b in zip(seen[0], seen[1]))


def test_key_runs_then_batched_top_k(G):
    """The offsets key runs writes, consumed on the device: the 3 largest values of every run of equal keys."""
    import torch

    rng = np.random.default_rng(192)
    n = 50000
    run_keys = np.sort(rng.integers(0, 900, n, dtype=np.uint32))
    values = random_keys(rng, "float32", n)
    runs = G.KeyRuns()
    d_keys, d_values = torch.from_numpy(run_keys.view(np.int32)).cuda(), torch.from_numpy(values.view(np.int32)).cuda()
    d_unique, d_offsets, d_count = (torch.zeros(n + 1, dtype=torch.int32, device="cuda") for _ in range(3))
    runs.run_ptr(d_keys.data_ptr(), n, d_offsets.data_ptr(), n, d_count.data_ptr(), unique_keys_ptr=d_unique.data_ptr(), stream=stream())
    sync()
    nruns = int(d_count[0].item())
    offsets = np.concatenate([[0], np.flatnonzero(np.diff(run_keys)) + 1, [n]])
    assert nruns == len(offsets) - 1
    ok, oi = Array.poisoned(nruns * 3 * 4), Array.poisoned(nruns * 3 * 4)
    G.TopK().run_batch_offsets_ptr(d_values.data_ptr(), n, d_offsets.data_ptr(), nruns, 3, ok.ptr, oi.ptr, key_type="float32", largest=True,
                                   stream=stream())
    sync()
    ek, ei, _ = expected(values, clamp_segments(offsets, n), 3, True, True)
    assert (ok.result(np.uint32) == ek).all() and (oi.result(np.uint32) == ei).all()


@pytest.mark.parametrize("dtype", ("int32", "uint64"))
def test_rows_equal_the_single_call(G, dtype):
    rng = np.random.default_rng(193)
    kb = np.dtype(dtype).itemsize
    top, single = G.TopK(), G.TopK()
    for n, k in ((300, 20), (5000, 300), (70000, 1000)):
        keys = random_keys(rng, dtype, 5 * n)
        ka = Array(keys)
        for largest, sorted_ in COMBOS:
            ok, oi, ot = Array.poisoned(5 * k * kb), Array.poisoned(5 * k * 4), Array.poisoned(5 * kb)
            top.run_batch_ptr(ka.ptr, n, 5, k, ok.ptr, oi.ptr, ot.ptr, key_type=dtype, largest=largest, sorted=sorted_, stream=stream())
            sk, si, st = Array.poisoned(5 * k * kb), Array.poisoned(5 * k * 4), Array.poisoned(5 * kb)
            for p in range(5):
                single.run_ptr(ka.ptr + p * n * kb, n, k, sk.ptr + p * k * kb, si.ptr + p * k * 4, st.ptr + p * kb, key_type=dtype, largest=largest,
                               sorted=sorted_, stream=stream())
            sync()
            for a, b in ((ok, sk), (oi, si), (ot, st)):
                assert (a.result(np.uint8) == b.result(np.uint8)).all(), (dtype, n, k, largest, sorted_)


# ------------------------------------------------------------------------------------------------------------------ refusals


def test_refusals_name_their_argument_and_write_nothing(G):
    rng = np.random.default_rng(194)
    keys = random_keys(rng, "uint32", 4096)
    ka, oa = Array(keys), Array(np.arange(0, 4097, 256, dtype=np.uint32))
    ok, oi, ot = Array.poisoned(16 * 8 * 4), Array.poisoned(16 * 8 * 4), Array.poisoned(16 * 4)
    top = G.TopK()

    def refused(words, fn, *args, **kwargs):
        with pytest.raises(G.GluError) as e:
            fn(*args, **kwargs)
        assert all(w in str(e.value) for w in words), (words, str(e.value))

    off, eq = top.run_batch_offsets_ptr, top.run_batch_ptr
    refused(["all NULL"], off, ka.ptr, 4096, oa.ptr, 16, 8)
    refused(["all NULL"], eq, ka.ptr, 256, 16, 8)
    refused(["k must not exceed count"], eq, ka.ptr, 256, 16, 257, ok.ptr)
    refused(["num_segments", "2^24"], off, ka.ptr, 4096, oa.ptr, (1 << 24) + 1, 8, ok.ptr)
    refused(["num_segments * k"], off, ka.ptr, 4096, oa.ptr, 1 << 20, 1 << 12, ok.ptr)
    refused(["2^32"], off, ka.ptr, 1 << 32, oa.ptr, 16, 8, ok.ptr)
    refused(["2^32"], eq, ka.ptr, 1 << 20, 1 << 12, 8, ok.ptr)
    refused(["offsets"], off, ka.ptr, 4096, None, 16, 8, ok.ptr)
    refused(["offsets", "aligned"], off, ka.ptr, 4096, oa.ptr + 2, 16, 8, ok.ptr)
    refused(["keys", "aligned"], off, ka.ptr + 2, 4000, oa.ptr, 16, 8, ok.ptr)
    refused(["out_keys", "aligned"], off, ka.ptr, 4096, oa.ptr, 16, 8, ok.ptr + 1)
    refused(["out_indices", "aligned"], off, ka.ptr, 4096, oa.ptr, 16, 8, None, oi.ptr + 2)
    refused(["out_kth", "aligned"], eq, ka.ptr, 256, 16, 8, None, None, ot.ptr + 2, key_type="uint32")
    refused(["keys buffer"], eq, None, 256, 16, 8, ok.ptr)
    refused(["out_keys overlaps keys"], off, ka.ptr, 4096, oa.ptr, 16, 8, ka.ptr + 64)
    refused(["out_indices overlaps the offsets array"], off, ka.ptr, 4096, oa.ptr, 16, 8, None, oa.ptr)
    refused(["out_indices overlaps out_keys"], eq, ka.ptr, 256, 16, 8, ok.ptr, ok.ptr + 16)
    refused(["out_kth overlaps out_keys"], eq, ka.ptr, 256, 16, 8, ok.ptr, None, ok.ptr + 16 * 8 * 4 - 4)
    refused(["BATCH_LOOP_MIN"], top.set_option, "BATCH_LOOP_MIN", -1)
    refused(["loop_min"], G.plan_top_k_batch, 100, 4, 3, loop_min=1 << 32)
    sync()
    for a in (ok, oi, ot):
        assert (a.result(np.uint8) == POISON).all()
    assert (ka.result(np.uint32) == keys).all()


# ------------------------------------------------------------------------------------------------------------------ wide indices


@pytest.mark.parametrize("dtype", ("uint32", "uint64"))
def test_segments_around_2_31_elements_and_4_gib(G, dtype):
    """uint32 keys around element 2^31, uint64 keys around byte 2^32: about 2000 segments of all classes on both sides of the boundary,
    inputs made on the device from a closed form, expected rows from torch on slices."""
    import torch

    kb = np.dtype(dtype).itemsize
    boundary = (1 << 31) if kb == 4 else (1 << 32) // 8
    rng = np.random.default_rng(195)
    limits = G.plan_top_k_batch(1, 1, 1, dtype)["limits"]
    lengths = mixed_lengths(rng, limits, 2000)
    first = boundary - int(lengths[:1000].sum()) - 1  # (odd or even as it comes; segment 1000 straddles or touches the boundary)
    offsets = offsets_of(lengths, first)
    total = int(offsets[-1]) + 3
    assert first > 0 and offsets[900] < boundary < offsets[1100] and total < 1 << 32
    tdt = torch.int32 if kb == 4 else torch.int64
    d_keys = torch.empty(total, dtype=tdt, device="cuda")
    lo = first - 8
    i = torch.arange(lo, total, dtype=torch.int64, device="cuda")
    d_keys[lo:] = ((i * 2654435761) % 1000003 + (i % 7) * 1000003).to(tdt)  # non-negative: unsigned order is signed order
    del i
    d_off = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    k = 24
    top = G.TopK()
    ok, oi, ot = Array.poisoned(2000 * k * kb), Array.poisoned(2000 * k * 4), Array.poisoned(2000 * kb)
    top.run_batch_offsets_ptr(d_keys.data_ptr(), total, d_off.data_ptr(), 2000, k, ok.ptr, oi.ptr, ot.ptr, key_type=dtype, largest=True, sorted=True,
                              stream=stream())
    sync()
    u = np.dtype("uint%d" % (8 * kb))
    got_k, got_i, got_t = ok.result(u).reshape(2000, k), oi.result(np.uint32).reshape(2000, k), ot.result(u)
    want = classes_of(G, clamp_segments(offsets, total), dtype)
    last = top.read_batch()
    assert {c: last[c] for c in want} == want and min(want.values()) > 0
    for s in range(2000):
        b, n = int(offsets[s]), int(lengths[s])
        ks = min(k, n)
        if n:
            v, idx = torch.sort(d_keys[b:b + n], descending=True, stable=True)
            assert (got_k[s, :ks] == v[:ks].cpu().numpy().view(u)).all() and (got_i[s, :ks] == idx[:ks].cpu().numpy()).all(), s
            assert got_t[s] == got_k[s, ks - 1]
        else:
            assert got_t[s] == poison_of(u)
        assert (got_k[s, ks:] == poison_of(u)).all() and (got_i[s, ks:] == POISON32).all(), s


# ------------------------------------------------------------------------------------------------------------------ the C++ program


def test_cpp_program(G):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_top_k_batch_api")
    assert os.path.exists(exe), "build() makes the C++ test programs"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
