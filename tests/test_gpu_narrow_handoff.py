"""GPU parity tests of the narrow hand-off: a sort of untyped 32-bit keys with values that ends in LDS, with
no run longer than the tile and the bucket round ordering the runs, hands its in-LDS pass the low 16 bits of every key in a side array
of 2-byte keys; the in-LDS pass rebuilds the other key bits from the run number.  Every other sort hands over whole keys, as before.
Which hand-off ran is read_handoff()["narrow"]; every result is compared bit for bit with oracle.stable_sort_pairs.

Sizes.  A sort makes the attempt to end in LDS only with a device-side plan, from 2^22 elements (a compile-time constant, no switch), so
every input here has 2^22 + 54321 pairs or a few more, with GLU_HIP_SORT_PAIR_MIN=1 and GLU_HIP_SORT_FINISH_MIN=1 as in
test_gpu_lds_finish.py.  The larger tiles are chosen through the longest run (GLU_HIP_SORT_LONG_RUNS=0: the longest run decides the
tile, and nothing goes to the long-run passes): a planted run of 2000 pairs takes 256 x 10, one of 4000 takes 256 x 18.  The 512 x 18
tile is enqueued only from 86 M pairs up (finish_geometry_for): its case has 2^27 + 333 pairs, drawn and checked on the device -- sorted,
every value pointing at its key, equal keys in input order: the three together are the stable sort, so the check is the oracle's.
Runs of 0, 1 and 2 pairs: 65536 runs cannot all be that short at 2^22 pairs, so a thousand runs of about 4100 pairs hold most of the
input and 2^16 .. 2^17 pairs are spread over the other 64536 runs."""
import functools
import gc

import numpy as np
import pytest

import oracle as O
import test_gpu_sort_bounds as sb

pytestmark = pytest.mark.gpu

SMALL = dict(GLU_HIP_SORT_PAIR_MIN=1, GLU_HIP_SORT_FINISH_MIN=1)
N = (1 << 22) + 54321


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def _sorter(G, **options):
    return G.RadixSort(options=dict(SMALL, **options))


def _run(G, sorter, keys, vals):
    kb, vb = G.ShaderStorageBuffer(keys), G.ShaderStorageBuffer(vals)
    sorter(kb, vb, keys.size)
    G.synchronize()
    return kb.get_data(np.uint32), vb.get_data(np.uint32), sorter.read_finish(), sorter.read_handoff()["narrow"]


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint32)


def _with_one_run_of(n, length, seed, run=0x1234):
    """Uniform keys, except that exactly `length` of them (at random positions) have the top 16 bits `run`."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2**32, n, dtype=np.uint32)
    keys[(keys >> 16) == run] ^= np.uint32(0x80000000)
    pos = rng.choice(n, size=length, replace=False)
    keys[pos] = (np.uint32(run) << 16) | rng.integers(0, 65536, length, dtype=np.uint32)
    return keys


def _sparse_runs(n, seed):
    """A thousand runs of about (n - 90000) / 1000 pairs (every 64th run from run 7 on), and 90000 pairs drawn over the other runs:
    most runs hold 0, 1 or 2 pairs.  Run 0 and run 65535 get exactly one pair each, the array's first and last elements among the
    positions."""
    rng = np.random.default_rng(seed)
    fat = (np.arange(1000, dtype=np.uint32) * np.uint32(64) + np.uint32(7))
    top = fat[rng.integers(0, 1000, n)]
    thin = rng.choice(n, 90000, replace=False)
    others = np.setdiff1d(np.arange(1, 65535, dtype=np.uint32), fat)
    top[thin] = others[rng.integers(0, others.size, thin.size)]
    top[0], top[n - 1] = 65535, 0
    return (top << np.uint32(16)) | rng.integers(0, 65536, n, dtype=np.uint32)


def _crowded(n, seed, every, distinct):
    """Runs of `distinct` low halves, drawn per run (so that all 16 low bits vary over the input): every run, or one run in
    `every`; the other runs have uniform low halves."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, 65536, n, dtype=np.uint32)
    low = rng.integers(0, 65536, n, dtype=np.uint32)
    palette = rng.integers(0, 65536, (65536, distinct), dtype=np.uint32)
    crowded = (top % np.uint32(every)) == 0
    low[crowded] = palette[top[crowded], rng.integers(0, distinct, int(crowded.sum()))]
    return (top << np.uint32(16)) | low


@functools.lru_cache(maxsize=None)
def _case(name):
    """(keys, values, expected keys, expected values) of a named input: drawn and sorted by the oracle once, read-only."""
    keys = {
        "uniform": lambda: _uniform(N, 1),
        "tile_256x10": lambda: _with_one_run_of(N, 2000, 2),
        "tile_256x18": lambda: _with_one_run_of(N, 4000, 3),
        "bits28": lambda: _uniform(N, 4) >> np.uint32(4),
        "bits28_under_constant_bits": lambda: (_uniform(N, 5) >> np.uint32(4)) | np.uint32(0xA0000000),
        "bits24": lambda: _uniform(N, 6) >> np.uint32(8),
        "all_runs_crowded": lambda: _crowded(N, 7, 1, 2),
        "one_run_in_16_crowded": lambda: _crowded(N, 8, 16, 3),
        "one_long_run": lambda: _with_one_run_of(N, 4608 + 5000, 9),
        "all_equal": lambda: np.full(N, 0x00C0FFEE, dtype=np.uint32),
        "sparse+0": lambda: _sparse_runs(N - N % 64, 10),
        "sparse+1": lambda: _sparse_runs(N - N % 64 + 1, 11),
        "sparse+4": lambda: _sparse_runs(N - N % 64 + 4, 12),
        "sparse+8": lambda: _sparse_runs(N - N % 64 + 8, 13),
    }[name]()
    vals = np.arange(keys.size, dtype=np.uint32)
    ek, ev = O.stable_sort_pairs(keys, vals)
    for a in (keys, vals, ek, ev):
        a.setflags(write=False)
    return keys, vals, ek, ev


def _check(name, gk, gv):
    _, _, ek, ev = _case(name)
    assert (gk == ek).all(), "%s: keys differ from the oracle at %s" % (name, np.flatnonzero(gk != ek)[:5])
    assert (gv == ev).all(), "%s: values differ from the oracle at %s" % (name, np.flatnonzero(gv != ev)[:5])


# what each input must come to: (options beyond SMALL, accepted, tile, narrow)
LONGEST_DECIDES = dict(GLU_HIP_SORT_LONG_RUNS=0)
OUTCOME = {
    "uniform": ({}, 1, 1536, 1),
    "tile_256x10": (LONGEST_DECIDES, 1, 2560, 1),
    "tile_256x18": (LONGEST_DECIDES, 1, 4608, 1),
}


@pytest.mark.parametrize("name", sorted(OUTCOME))
def test_uniform_keys_take_the_narrow_handoff_in_every_tile(G, name):
    options, accepted, capacity, narrow = OUTCOME[name]
    keys, vals, _, _ = _case(name)
    s = _sorter(G, **options)
    gk, gv, fin, took = _run(G, s, keys, vals)
    _check(name, gk, gv)
    assert fin["attempted"] == 1 and fin["accepted"] == accepted and fin["capacity"] == capacity, fin
    assert took == narrow
    # the option at 0: whole keys in the key array, the same arrays, and no side array (n x 2 bytes less scratch)
    wide = _sorter(G, GLU_HIP_SORT_NARROW_HANDOFF=0, **options)
    gk2, gv2, fin2, took2 = _run(G, wide, keys, vals)
    assert (gk2 == gk).all() and (gv2 == gv).all()
    assert took2 == 0 and fin2 == fin
    assert s.scratch_size() - wide.scratch_size() == 2 * keys.size


def test_the_largest_tile(G):
    """512 x 18: 2^27 + 333 pairs (the size from which that tile is enqueued) with one run of 9000, the longest run deciding."""
    import torch

    n = (1 << 27) + 333
    s = G.RadixSort(options=LONGEST_DECIDES)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    keys = torch.randint(-2**31, 2**31, (n,), dtype=torch.int32, device="cuda:0", generator=g)
    run = torch.tensor(0x1234 << 16, dtype=torch.int32, device="cuda:0")
    keys[(keys >> 16) == 0x1234] ^= torch.tensor(0x40000000, dtype=torch.int32, device="cuda:0")
    pos = torch.randperm(n, device="cuda:0", generator=g)[:9000]
    keys[pos] = run | (keys[pos] & 0xFFFF)
    vals = torch.arange(n, dtype=torch.int32, device="cuda:0")
    k0 = keys.clone()
    torch.cuda.synchronize()
    s.run_ptr(keys.data_ptr(), vals.data_ptr(), n)
    G.synchronize()
    fin = s.read_finish()
    assert fin["attempted"] == 1 and fin["accepted"] == 1 and fin["capacity"] == 9216 and fin["longest_run"] == 9000, fin
    assert s.read_handoff()["narrow"] == 1
    flipped = keys ^ torch.tensor(-2**31, dtype=torch.int32, device="cuda:0")  # (unsigned order == order of key ^ 0x80000000 as int32)
    assert bool((flipped[1:] >= flipped[:-1]).all()), "not sorted"
    assert bool((k0[vals.long()] == keys).all()), "a value does not point at its key"
    eq = keys[1:] == keys[:-1]
    assert bool((vals[1:][eq] > vals[:-1][eq]).all()), "equal keys out of input order"
    del keys, vals, k0, flipped, eq
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["sparse+0", "sparse+1", "sparse+4", "sparse+8"])
def test_runs_of_one_and_empty_runs(G, name):
    """Most runs hold 0, 1 or 2 pairs -- their starts meet every alignment of a 64-element line of 2-byte keys --, the first and the
    last run hold one pair each, and the count is a multiple of 64, odd, a multiple of 4 but not of 8, of 8 but not of 64: the key of
    a run of one is widened and written, and the array's last piece is ragged."""
    keys, vals, _, _ = _case(name)
    lengths = np.bincount(keys >> 16, minlength=65536)
    assert (lengths <= 2).sum() > 40000 and (lengths == 1).sum() > 10000 and (lengths == 0).sum() > 5000
    assert lengths[0] == 1 and lengths[65535] == 1 and lengths.max() <= 4608
    gk, gv, fin, took = _run(G, _sorter(G, **LONGEST_DECIDES), keys, vals)
    _check(name, gk, gv)
    assert fin["accepted"] == 1 and fin["capacity"] == 4608 and took == 1, fin


@pytest.mark.parametrize("name", ["bits28", "bits28_under_constant_bits"])
def test_28_bit_keys(G, name):
    """The runs are key bits [12, 28), 12 bits are left to order: the upper bits come from the run number at a shifted top bit, and
    from the bits no key differs in."""
    keys, vals, _, _ = _case(name)
    gk, gv, fin, took = _run(G, _sorter(G), keys, vals)
    _check(name, gk, gv)
    assert fin["accepted"] == 1 and fin["top_bit"] == 28 and took == 1, fin


def test_24_bit_keys_keep_the_whole_keys(G):
    """Eight bits left to order: the ballot rounds take every run, and they read whole keys."""
    keys, vals, _, _ = _case("bits24")
    gk, gv, fin, took = _run(G, _sorter(G), keys, vals)
    _check("bits24", gk, gv)
    assert fin["accepted"] == 1 and fin["top_bit"] == 24 and took == 0, fin


@pytest.mark.parametrize("name", ["all_runs_crowded", "one_run_in_16_crowded"])
def test_crowded_runs(G, name):
    """Two distinct low halves in every run, or three in one run of 16: the bucket kernel lists such a run for the ballot rounds, and in narrow mode writes its
    widened keys first.  The values of equal keys stay in input order (the oracle's).
    That the bail-out is taken (the library reports no count of crowded runs): a run holds 65 pairs on average, in the 256 x 6 tile a
    bucket is the top 10 of the 16 low key bits, and a run's two (three) low halves fall into two (three) buckets of about 32 (21)
    words each.  A word that finds kBucketMaxLen = 24 others in its bucket, or a wave whose first words put eight into one bucket,
    sends the run to the ballot rounds: nearly every run of the first input and a good part of the crowded runs of the second.  Without
    the widening loop those runs would come out with the keys the caller's array held before the in-LDS pass, and the oracle differs."""
    keys, vals, _, _ = _case(name)
    gk, gv, fin, took = _run(G, _sorter(G), keys, vals)
    _check(name, gk, gv)
    assert fin["accepted"] == 1 and took == 1, fin


def test_a_run_longer_than_the_largest_tile_keeps_the_whole_keys(G):
    keys, vals, _, _ = _case("one_long_run")
    s = _sorter(G)
    gk, gv, fin, took = _run(G, s, keys, vals)
    _check("one_long_run", gk, gv)
    assert fin["accepted"] == 1 and s.read_long_runs()["runs"] == 1 and took == 0, fin


ROUND = [("uniform", 1, 1), ("one_long_run", 1, 0), ("all_equal", 0, 0)]


def test_one_object_alternates(G):
    """Narrow, wide (a long run) and refused inputs in turn, twice round, on one object."""
    s = _sorter(G, GLU_HIP_SORT_FINISH_BACKOFF=0)
    for name, accepted, narrow in ROUND * 2:
        keys, vals, _, _ = _case(name)
        gk, gv, fin, took = _run(G, s, keys, vals)
        _check(name, gk, gv)
        assert fin["attempted"] == 1 and fin["accepted"] == accepted and took == narrow, (name, fin, took)


def test_one_captured_graph_serves_both_handoffs(G):
    """Which form of the second scatter runs is decided on the device: one captured graph of a sort replays over the same three
    inputs, twice round."""
    import torch

    sorter = _sorter(G, GLU_HIP_SORT_FINISH_BACKOFF=0)
    sorter.prepare_internal_buffers(N)
    kt = torch.empty(N, dtype=torch.int32, device="cuda")
    vt = torch.empty(N, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        kt.copy_(torch.from_numpy(_case("uniform")[0].view(np.int32).copy()))  # (the cases are read-only arrays: torch wants writable ones)
        vt.copy_(torch.from_numpy(_case("uniform")[1].view(np.int32).copy()))
        sorter.run_ptr(kt.data_ptr(), vt.data_ptr(), N, 0, side.cuda_stream)  # warm-up outside the capture
        side.synchronize()
        gc.collect()  # (an operator object that dies inside the capture would wait for the device there)
        with torch.cuda.graph(graph, stream=side):
            sorter.run_ptr(kt.data_ptr(), vt.data_ptr(), N, 0, torch.cuda.current_stream().cuda_stream)
        for name, accepted, narrow in ROUND * 2:
            keys, vals, _, _ = _case(name)
            kt.copy_(torch.from_numpy(keys.view(np.int32).copy()))
            vt.copy_(torch.from_numpy(vals.view(np.int32).copy()))
            graph.replay()
            side.synchronize()
            _check(name, kt.cpu().numpy().view(np.uint32), vt.cpu().numpy().view(np.uint32))
            fin = sorter.read_finish()
            assert fin["accepted"] == accepted and sorter.read_handoff()["narrow"] == narrow, (name, fin)


@pytest.mark.parametrize("place", [(16, 48), (112, 16)], ids=["k16v48", "k112v16"])
def test_arrays_inside_larger_buffers_keep_their_guard_bands(G, place):
    """The caller's arrays 16-byte but not 128-byte aligned, poison on both sides of both: a narrow sort writes none of it."""
    keys, vals = sb.scrub(_case("uniform")[0]), sb.iota(N)
    order = sb.stable_order(keys)
    ka, va = sb.Array(keys, place[0]), sb.Array(vals, place[1])
    assert ka.ptr % 128 == place[0] and va.ptr % 128 == place[1]
    s = _sorter(G)
    sb.sync()
    s.run_ptr(ka.ptr, va.ptr, N, 0, sb.stream())
    sb.sync()
    ka.expect(keys[order], "keys")
    va.expect(vals[order], "values")
    assert s.read_finish()["accepted"] == 1 and s.read_handoff()["narrow"] == 1


# uniform keys in every tile; runs of one pair, empty runs and every ragged count; 28-bit keys, with and without constant bits above them
FILLED = dict(OUTCOME)
FILLED.update({name: (LONGEST_DECIDES, 1, 4608, 1) for name in ("sparse+0", "sparse+1", "sparse+4", "sparse+8")})
FILLED.update({name: ({}, 1, 1536, 1) for name in ("bits28", "bits28_under_constant_bits")})


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
@pytest.mark.parametrize("name", sorted(FILLED))
def test_fresh_scratch_of_any_content(G, monkeypatch, name, fill):
    """GLU_HIP_SCRATCH_FILL: the side array and everything else the object allocates hold that byte before the sort; every element the
    in-LDS pass reads from the side array was written by this call's narrow scatter -- the one key of a run of one pair, the pieces in
    front of and behind every run at every alignment, the array's ragged last piece, and the common upper bits of 28-bit keys come
    out right whatever the scratch held."""
    options, accepted, capacity, narrow = FILLED[name]
    keys, vals, _, _ = _case(name)
    monkeypatch.setenv("GLU_HIP_SCRATCH_FILL", str(fill))
    before = G.scratch_filled_bytes()
    s = _sorter(G, **options)
    gk, gv, fin, took = _run(G, s, keys, vals)
    assert G.scratch_filled_bytes() - before >= s.scratch_size() > 2 * keys.size
    _check(name, gk, gv)
    assert fin["accepted"] == accepted and fin["capacity"] == capacity and took == narrow, fin


def test_profile_books_the_form_that_moved_the_data(G):
    """read_profile books, as the scatter of the second top-bit pass, the launch that ran and not the form beside it that returned at
    once.  Five sorts of the same uniform keys a window, after one to warm up, on an object with the option at 1 and on one with it at
    0: both book two passes and one in-LDS pass a sort.  The narrow sort's two scatters move 30 of the other's 32 bytes per pair, so its
    scatter time is about that share of the other's; with the interval of the wrong form booked for the second scatter it would be
    about half.  The bound lies between the two, a quarter off either."""
    keys, vals, _, _ = _case("uniform")
    booked = {}
    for option in (1, 0):
        s = _sorter(G, GLU_HIP_SORT_NARROW_HANDOFF=option)
        s.set_profiling(True)
        _run(G, s, keys, vals)
        s.read_profile()
        for _ in range(5):
            gk, gv, fin, took = _run(G, s, keys, vals)
            assert took == option and fin["accepted"] == 1
        _check("uniform", gk, gv)
        booked[option] = s.read_profile()
        assert booked[option]["passes"] == 10 and booked[option]["finish_passes"] == 5, booked[option]
    print("scatter_ms of five sorts: narrow %.4f, whole keys %.4f" % (booked[1]["scatter_ms"], booked[0]["scatter_ms"]))
    assert 0.72 * booked[0]["scatter_ms"] < booked[1]["scatter_ms"] < 1.2 * booked[0]["scatter_ms"], booked
