"""GPU tests that no operator reads scratch it has not written in that call.  What an operator object's scratch holds when it is
allocated is an input of every kernel that no caller controls: GLU_HIP_SCRATCH_FILL fills every new scratch
allocation with a byte, and glu_scratch_filled_bytes says how many bytes were filled.  DESIGN.md, "Who writes scratch first", is
the reading these tests confirm.

A case is one call, or one documented call sequence, on FRESH objects: made after the variable is set, never prepared before.  Every
case runs under the fills 0x00 (what fresh memory usually holds: the control, which proves the case's own reference right), 0xFF (every
counter, offset and flag all-ones; a NaN as a float) and 0x5A (a plausible count, a large finite float), in that order.  Under each
fill the operator's own test module checks the case: every output against numpy, the poison around every array, the path from the
object's reports.  Across the fills the reports, and the outputs that are held to a bound and not to `==`, are the same bits.  The
fill counter grows by at least the scratch the object holds (the plan's bytes, or the sort's own account), and does not move for
the two operators that own no scratch.  Operators with a prepare run both ways: prepare then the call, and the call alone.

Tiles and class limits come from the plan functions; the checkers and references are the other modules'."""
import os

import numpy as np
import pytest

import exact_inputs as X
import scan_ops_cases as sc
import test_gpu_batched_reduce as br
import test_gpu_batched_scan as bs
import test_gpu_batched_sort as bsort
import test_gpu_expand as ex
import test_gpu_gather as ga
import test_gpu_histogram as hi
import test_gpu_histogram_batch as hb
import test_gpu_key_runs as kr
import test_gpu_merge as mg
import test_gpu_scan_ops as so
import test_gpu_scan_reduce_types as srt
import test_gpu_select as se
import test_gpu_set_ops as st
import test_gpu_sort_bounds as sb
import test_gpu_sorted_search as ss
import test_gpu_sorted_search_batch as ssb
import test_gpu_top_k as tk
import test_gpu_top_k_batch as tkb
from test_top_k_pick import key_code

pytestmark = pytest.mark.gpu
ENV = "GLU_HIP_SCRATCH_FILL"
FILLS = (0x00, 0xFF, 0x5A)
BOTH_WAYS = pytest.mark.parametrize("prepared", [False, True], ids=["grows_in_the_call", "prepared"])
SOME = 1  # the scratch an object holds where no plan states its bytes: the counter must move


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def frozen(value):
    """A report or an array as something `==` compares bit for bit."""
    if isinstance(value, np.ndarray):
        return (str(value.dtype), value.shape, np.ascontiguousarray(value).tobytes())
    if isinstance(value, dict):
        return {k: frozen(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return tuple(frozen(v) for v in value)
    return value


def under_every_fill(G, monkeypatch, case, moves=True):
    """case() makes its objects, runs and checks the call, and returns (held, told): the scratch bytes the objects hold at the least,
    and what is compared across the fills.  moves: True, the counter grows by `held` > 0 at least; False, it does not move; None,
    the case allocates only where `held` says so (a path that needs no scratch)."""
    seen = []
    for fill in FILLS:
        monkeypatch.setenv(ENV, str(fill))
        before = G.scratch_filled_bytes()
        held, told = case()
        sb.sync()
        grew = G.scratch_filled_bytes() - before
        if moves is False:
            assert grew == 0, "fill 0x%02X: an operator without scratch filled %d bytes" % (fill, grew)
        else:
            assert grew >= held and (moves is None or held > 0), "fill 0x%02X: %d bytes filled, the object holds %d" % (fill, grew, held)
        seen.append(frozen(told))
    for fill, told in zip(FILLS[1:], seen[1:]):
        assert told.keys() == seen[0].keys()
        for name in told:
            assert told[name] == seen[0][name], "fill 0x%02X: %s differs from what it is after a fill of zeros" % (fill, name)


def test_the_switch_is_read_at_every_growth_and_refuses_what_is_no_byte(G, monkeypatch):
    """Unset: nothing is filled.  Set between two growths of one object: the second is filled.  256, -1, 0x100, a word and a number
    with a blank behind it: an invalid argument of the call that grows, after which the object holds no allocation and a call under a
    good value grows again."""
    monkeypatch.delenv(ENV, raising=False)
    before = G.scratch_filled_bytes()
    scan = G.BlellochScan(G.DataType_Uint)
    scan.prepare_batch(1000, 10)
    assert G.scratch_filled_bytes() == before
    monkeypatch.setenv(ENV, "0x5A")
    scan.prepare_batch(100000, 10)
    grown = G.scratch_filled_bytes() - before
    assert grown > 0
    scan.prepare_batch(100000, 10)  # (no growth: no fill)
    assert G.scratch_filled_bytes() - before == grown
    for bad in ("256", "-1", "0x100", "fill", "12 "):
        monkeypatch.setenv(ENV, bad)
        runs = G.KeyRuns()
        with pytest.raises(G.GluError) as e:
            runs.prepare(5000, 32)
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT and ENV in e.value.message and "0 .. 255" in e.value.message, e.value.message
        assert G.scratch_filled_bytes() - before == grown
        monkeypatch.setenv(ENV, "255")
        kr.check_case(G, runs, kr.widen(np.arange(5000) // 3, np.uint32), 5000)
        assert G.scratch_filled_bytes() - before > grown
        grown = G.scratch_filled_bytes() - before
        runs.destroy()  # (the refusal's traceback keeps this frame, and with it the objects, until a collection: end them here)
    scan.destroy()


# ---------------------------------------------------------------------------------------------------------------------------- sort


def sort_told(sorter, sorted_before=True):
    """Every report a sort object offers that is no time (read_plan is an invalid state before the object's first sort)."""
    told = {"finish": sorter.read_finish(), "long_runs": sorter.read_long_runs(), "seg_finish": sorter.read_seg_finish(),
            "batch": sorter.read_batch(), "scratch": sorter.scratch_size()}
    if sorted_before:
        told["plan"] = sorter.read_plan(8, roles=True)
    return told


SINGLE_SORTS = {
    "one_workgroup": (5000, None, {}, 1),
    "mid_size_digit8_fused": (70001, 8, dict(SORT_NO_FUSED_SCAN=0), 4),
    "mid_size_digit8_unfused": (70001, 8, dict(SORT_NO_FUSED_SCAN=1), 4),
    "mid_size_digit4_fused": (70001, 4, dict(SORT_NO_FUSED_SCAN=0), 8),
    "mid_size_digit4_unfused": (70001, 4, dict(SORT_NO_FUSED_SCAN=1), 8),
    "line_scatter": (123457, None, dict(SORT_LARGE_MIN=1), 4),
}


@BOTH_WAYS
@pytest.mark.parametrize("name", sorted(SINGLE_SORTS))
def test_sorts_below_the_planned_size(G, monkeypatch, name, prepared):
    """One workgroup; count, row scan (launched, or the scatter's prologue) and scatter of the small geometry (`table`); the 128-byte
    line scatter.  The passes are the profile's: one for the single workgroup, one per digit behind it."""
    n, digit, options, passes = SINGLE_SORTS[name]
    keys, order = sb.uniform_keys(4, n), sb.uniform_order(4, n)

    def case():
        sorter = sb.profiled(G, digit_bits=digit, **options)
        if prepared:
            sorter.prepare_internal_buffers(n, 4, True)
        sb.sort_in_place(keys, order, (0, 0), sb.untyped_call(sorter, n, 4, True))
        assert sorter.read_profile()["passes"] == passes
        return sorter.scratch_size(), sort_told(sorter)

    under_every_fill(G, monkeypatch, case)


PLANNED = [(shape, "u32pairs") for shape in ("uniform", "range20", "two_long_runs", "few17", "all_equal", "zeros10")]
PLANNED += [(shape, kind) for kind in ("u64pairs", "float32", "u32keys") for shape in ("uniform", "two_long_runs")]


@BOTH_WAYS
@pytest.mark.parametrize("shape,kind", PLANNED, ids=["%s-%s" % c for c in PLANNED])
def test_planned_sorts(G, monkeypatch, shape, kind, prepared):
    """2^22 + 54321 elements, passes paired and the attempt to end in LDS made from that size: `plan`, `pair_t2`, `pair_table`,
    `pair_ranges`, `pair_wide`, the `finish_*` arrays, the `long_*` arrays; accepted, refused (all_equal), with runs for the segmented
    long-run passes, for every kind of key.  What ran is planned_sort's to assert from read_finish, read_long_runs and the pair roles."""
    keys = sb.planned_case(shape, kind)[0]
    with_vals = kind != "u32keys"

    def case():
        sorter = G.RadixSort(options=sb.PLANNED_OPTIONS)
        if prepared:
            sorter.prepare_internal_buffers(keys.size, keys.dtype.itemsize, with_vals)
        sb.planned_sort(G, sorter, shape, kind, (0, 0 if with_vals else None))
        return sorter.scratch_size(), sort_told(sorter)

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("shape", ["uniform", "two_long_runs"])
def test_planned_sorts_of_4_bit_digits(G, monkeypatch, shape, prepared):
    """The same size with 4-bit digits: eight passes in four pairs, the leader's table per sub-block (`pair_sub`); no attempt to end in
    LDS, which takes 8-bit digits."""
    keys, order, _ = sb.planned_case(shape, "u32pairs")

    def case():
        sorter = G.RadixSort(digit_bits=4, options=sb.PLANNED_OPTIONS)
        if prepared:
            sorter.prepare_internal_buffers(keys.size, 4, True)
        sb.sort_in_place(keys, order, (0, 0), sb.untyped_call(sorter, keys.size, 4, True))
        told = sort_told(sorter)
        assert told["finish"]["attempted"] == 0 and told["plan"][2] == [1, 2] * 4, told
        return sorter.scratch_size(), told

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
def test_sort_by_a_bit_range(G, monkeypatch, prepared):
    """Bits 8 to 20 of 300 001 pairs: two passes, the second of four bits."""
    n = 300001
    keys = sb.uniform_keys(4, n)
    order = sb.stable_order(keys, 8, 20)

    def case():
        sorter = sb.profiled(G)
        if prepared:
            sorter.prepare_internal_buffers(n, 4, True)
        sb.sort_in_place(keys, order, (0, 0), lambda k, v: sorter.sort_bit_range_ptr(k, v, n, 8, 20, sb.stream()))
        assert sorter.read_profile()["passes"] == sb.digit_passes(8, 20, 4, 8) == 2
        return sorter.scratch_size(), sort_told(sorter)

    under_every_fill(G, monkeypatch, case)


@pytest.mark.parametrize("with_histogram", [True, False], ids=["histogram", "no_histogram"])
def test_partition(G, monkeypatch, with_histogram):
    """partition_ptr reserves the table alone, in the call: one pass, the digit histogram copied out of the table's totals."""
    def case():
        sorter = sb.profiled(G)
        sb.partition(G, sorter, 200003, 13, 5, with_histogram, (0, 0, 0, 0))
        return sorter.scratch_size(), sort_told(sorter, sorted_before=False)

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("n", [65536, 700001])
def test_segmented_sort(G, monkeypatch, n, prepared):
    """run_segments_ptr by 32 bits: the segmented passes (`seg_desc`, the table per sub-block) and, at 700 001 elements, the attempt to
    end in LDS (`finish_starts`, `seg_gate`), which segmented_sort asserts from read_seg_finish."""
    def case():
        sorter = G.RadixSort()
        if prepared:
            sorter.prepare_internal_buffers(n, 4, True)
        rep = sb.segmented_sort(G, sorter, n, 32, ("aligned", 0))
        assert n != 700001 or (rep["attempted"], rep["accepted"]) == (1, 1), rep
        return sorter.scratch_size(), sort_told(sorter)

    under_every_fill(G, monkeypatch, case)


def batch_lengths(G, key_bytes):
    """Lengths of the wave, the block and the long class of the batched sort, an empty segment among them, by plan_batch."""
    lens = [0] + sb.BATCH_LENGTHS["wave"][:6] + sb.BATCH_LENGTHS["block"] + [0] + sb.BATCH_LENGTHS["long"]
    paths = [G.plan_batch(int(n), key_bytes)[0] for n in lens]
    assert min(paths.count(p) for p in (0, 1, 2, 3)) > 0
    return lens, {"wave": paths.count(1), "block": paths.count(2), "long": paths.count(3)}


@BOTH_WAYS
def test_batched_sort_of_offsets(G, monkeypatch, prepared):
    """One batch with segments of the wave, the block and the long class and two empty ones (`batch_lists`; the long class passes
    through the key and value scratch)."""
    lens, classes = batch_lengths(G, 4)
    head, tail = 777, 1234
    offsets = (np.concatenate([[0], np.cumsum(lens)]) + head).astype(np.uint32)
    total = int(offsets[-1]) + tail
    keys, vals = sb.uniform_keys(4, total, seed=3), sb.iota(total)
    ek, ev = bsort.expected(keys, vals, offsets)

    def case():
        sorter = G.RadixSort()
        if prepared:
            sorter.prepare_batch(total, len(lens), 4, True)
        ka, va, oa = sb.Array(keys), sb.Array(vals), sb.Array(offsets)
        sb.sync()
        sorter.sort_batch_offsets_ptr(ka.ptr, va.ptr, total, oa.ptr, len(lens), "uint32", sb.stream())
        sb.sync()
        ka.expect(ek, "keys")
        va.expect(ev, "values")
        oa.expect(offsets, "offsets")
        told = sort_told(sorter, sorted_before=False)
        assert told["batch"] == classes, told
        return sorter.scratch_size(), told

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("cls", ["wave", "block", "long"])
def test_batched_sort_of_equal_partitions(G, monkeypatch, cls, prepared):
    """Three equal partitions of one class: the host picks the kernel, no list is made."""
    count, parts = sb.BATCH_LENGTHS[cls][-1], 3
    assert G.plan_batch(count, 4)[0] == sb.BATCH_PATH[cls]
    keys, vals = sb.uniform_keys(4, count * parts, seed=5), sb.iota(count * parts)
    ek, ev = bsort.expected(keys, vals, np.arange(parts + 1) * count)

    def case():
        sorter = G.RadixSort()
        if prepared:
            sorter.prepare_batch(count * parts, parts, 4, True)
        ka, va = sb.Array(keys), sb.Array(vals)
        sb.sync()
        sorter.sort_batch_ptr(ka.ptr, va.ptr, count, parts, "uint32", sb.stream())
        sb.sync()
        ka.expect(ek, "keys")
        va.expect(ev, "values")
        told = sort_told(sorter, sorted_before=False)
        assert told["batch"] == {c: (parts if c == cls else 0) for c in ("wave", "block", "long")}, told
        return sorter.scratch_size(), told

    # (the wave and the block class sort inside LDS: an unprepared call of theirs reserves nothing, and nothing is filled)
    under_every_fill(G, monkeypatch, case, moves=True if prepared or cls == "long" else None)


# ------------------------------------------------------------------------------------------------------------------ scan and reduce

SCAN_COUNT = 3 * 32768 + 17


@BOTH_WAYS
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("chained", [2, 0])
def test_scan_of_uint32(G, monkeypatch, chained, parts, prepared):
    """3 x 32768 + 17 elements a partition: GLU_HIP_SCAN_CHAINED=2, the single-pass scan from two chunks up (`chain`, `ticket`); 0, the
    chunk sums and their scan (`sums`).  Inputs of exact sums, as test_gpu_scan_reduce_types.py draws them: `==`."""
    monkeypatch.setenv("GLU_HIP_SCAN_CHAINED", str(chained))
    dt, n = G.DataType_Uint, SCAN_COUNT * parts
    drawn = X.exact_sums(dt, n, X.seed_of(dt, n))
    want = X.expected_scan(drawn, SCAN_COUNT, parts)

    def case():
        scan = G.BlellochScan(dt)
        if prepared:
            scan.prepare(SCAN_COUNT, parts)
        srt.assert_same(srt.run_scan(G, scan, dt, drawn.data, SCAN_COUNT, parts), want, (dt, SCAN_COUNT, parts, chained))
        return SOME, {}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("chained", [2, 0])
def test_scan_of_floats_that_round(G, monkeypatch, chained, prepared):
    """The same shape in floats whose sums round, inside the bound of test_gpu_scan_reduce_types.py -- and the same bits under every
    fill."""
    monkeypatch.setenv("GLU_HIP_SCAN_CHAINED", str(chained))
    dt, n = G.DataType_Float, SCAN_COUNT
    data = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
    ref, bound = X.rounding_scan_reference(dt, data, SCAN_COUNT, 1)

    def case():
        scan = G.BlellochScan(dt)
        if prepared:
            scan.prepare(SCAN_COUNT, 1)
        got = srt.run_scan(G, scan, dt, data, SCAN_COUNT, 1)
        bad = np.flatnonzero(~X.within_bound(got, ref, bound))
        assert bad.size == 0, (chained, bad[:4].tolist())
        return SOME, {"scan": got}

    under_every_fill(G, monkeypatch, case)


@pytest.mark.parametrize("op", [X.OP_SUM, X.OP_MIN, X.OP_MAX])
def test_reduce_of_uint32(G, monkeypatch, op):
    """2^20 + 3 elements: two stages through `partials` (allocated when the object is made)."""
    dt, n = G.DataType_Uint, (1 << 20) + 3
    cases = list(srt.reduce_cases(dt, op, n, False))

    def case():
        told = {}
        for label, data, want in cases:
            got = srt.run_reduce(G, G.Reduce(dt, op), dt, data, n)
            assert (got == want).all(), (op, label, got.tolist(), want.tolist())
            told[str(label)] = got
        return SOME, told

    under_every_fill(G, monkeypatch, case)


def test_reduce_of_floats_that_round(G, monkeypatch):
    dt, n = G.DataType_Float, (1 << 20) + 3
    data = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
    ref, bound = X.rounding_sum_reference(dt, data)

    def case():
        got = srt.run_reduce(G, G.Reduce(dt, X.OP_SUM), dt, data, n)
        assert X.within_bound(got, ref, bound).all(), (got.tolist(), ref.tolist(), bound.tolist())
        return SOME, {"sum": got}

    under_every_fill(G, monkeypatch, case)


# ------------------------------------------------------------------------------------- batched reduce, batched scan, scan operators


@BOTH_WAYS
@pytest.mark.parametrize("dt,op", [(3, 0), (0, 0), (3, 3)], ids=["uint_sum", "float_sum", "uint_max"])
def test_batched_reduce(G, monkeypatch, dt, op, prepared):
    """An empty segment and one of each class, the long one of several chunks (`batch_lists`, `batch_partials`)."""
    wave, block = br.class_limits(G, 4)
    lens = [0, 3, wave, block, 2 * block + 5, 0]
    paths = [G.plan_reduce_batch(n, 4)[0] for n in lens]
    assert [paths.count(p) for p in (1, 2, 3)] == [2, 1, 1] and G.plan_reduce_batch(lens[4], 4)[1] >= 2
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total = int(offsets[-1])
    d = br.make_data(np.random.default_rng(dt * 4 + op), total, dt, op)
    want = br.expected_segments(d, dt, op, offsets)

    def case():
        red = G.Reduce(dt, op)
        if prepared:
            red.prepare_batch(total, len(lens))
        got = br.run_offsets(G, red, d, dt, offsets)
        assert (got == want).all(), (got, want)
        rb = red.read_batch()
        assert [rb["wave"], rb["block"], rb["long"]] == [2, 1, 1], rb
        return SOME, {"out": got, "batch": rb}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("dt", [3, 0], ids=["uint", "float"])
def test_batched_scan(G, monkeypatch, dt, prepared):
    wave, block, chunk = bs.class_limits(G, 4)
    lens = [0, 5, wave, block, 3 * chunk + 1, 0]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total = int(offsets[-1])
    d = bs.make_data(np.random.default_rng(40 + dt), dt, offsets, total)
    want = bs.expected_scan(d, dt, offsets)

    def case():
        scan = G.BlellochScan(dt)
        if prepared:
            scan.prepare_batch(total, len(lens))
        got = bs.run(G, scan, d, dt, offsets)
        assert bs.same_bits(got, want), bs.first_difference(got, want, offsets, 1)
        rb = scan.read_batch()
        assert [rb["wave"], rb["block"], rb["long"]] == [2, 1, 1], rb
        return SOME, {"out": got, "batch": rb}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("whole", [False, True], ids=["offsets", "whole_array"])
def test_scan_with_an_operator(G, monkeypatch, whole, prepared):
    """op=max, inclusive, into a second array, of floats: the batch of the classes, and the one-segment form with offsets == NULL, whose
    two offset words are written on the device (`batch_whole`)."""
    dt, op = 0, "max"
    wave, block, chunk, _ = so.class_limits(G, 4)
    lens = [3 * chunk + 1] if whole else [0, 5, wave, block, 3 * chunk + 1, 0]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total = int(offsets[-1])
    d = sc.make_data(np.random.default_rng(50 + whole), dt, op, offsets, total)
    want = sc.expected(d, dt, op, True, offsets, base=so.poison_like(d))

    def case():
        scan = G.BlellochScan(dt)
        if prepared:
            scan.prepare_batch(total, len(lens))
        got, after = so.scan_call(G, scan, d, dt, None if whole else offsets, op, True, True, whole=whole)
        assert sc.same(op, np.float32, got, want), sc.first_difference(got, want, 1)
        assert sc.same_bits(after, d), "data changed"
        rb = scan.read_batch()
        assert [rb["wave"], rb["block"], rb["long"]] == ([0, 0, 1] if whole else [2, 1, 1]), rb
        return SOME, {"out": got, "batch": rb}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
def test_scan_by_key(G, monkeypatch, prepared):
    """The running maximum by key through a fresh KeyRuns and a fresh BlellochScan, runs of every class."""
    def case():
        scan, runs = G.BlellochScan(G.DataType_Uint), G.KeyRuns()
        if prepared:
            runs.prepare(1 << 20, 32)
            scan.prepare_batch(1 << 20, 64)
        out, rb = so.running_maximum_by_key(G, scan, runs)
        return SOME, {"out": out, "batch": rb}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
def test_reduce_by_key(G, monkeypatch, prepared):
    """Sums by key through a fresh KeyRuns and a fresh Reduce: the offsets are key runs' (numpy's heads), the sums the batched
    reduce's over those offsets, the identity from the number of runs on."""
    wave, block = br.class_limits(G, 4)
    lens = [1, 2, wave, wave + 1, block, 2 * block + 5, 7]
    rng = np.random.default_rng(60)
    keys = np.repeat(np.sort(rng.choice(1 << 20, len(lens), replace=False)).astype(np.uint32), lens)
    n, max_runs = keys.size, len(lens) + 5
    vals = rng.integers(0, 2**32, n, dtype=np.uint32)
    want_offsets, want_unique, want_runs = kr.expected(keys, 0xFFFFFFFF, max_runs)
    want_sums = br.expected_segments(vals, 3, 0, want_offsets)[:, 0]
    assert want_runs == len(lens)

    def case():
        runs, red = G.KeyRuns(), G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum)
        if prepared:
            runs.prepare(n, 32)
            red.prepare_batch(n, max_runs)
        ka, va = kr.Array(keys), kr.Array(vals)
        oa, ua, na = kr.Array.poisoned(max_runs + 1, np.uint32), kr.Array.poisoned(max_runs, np.uint32), kr.Array.poisoned(1, np.uint32)
        out = kr.Array.poisoned(max_runs, np.uint32)
        sb.sync()
        red.run_by_key_ptr(runs, ka.ptr, va.ptr, out.ptr, n, oa.ptr, max_runs, na.ptr, ua.ptr, stream=kr.stream())
        sb.sync()
        assert int(na.result()[0]) == want_runs
        assert (oa.result() == want_offsets).all() and (ua.result() == want_unique).all()
        assert (out.result() == want_sums).all()
        assert (ka.result() == keys).all() and (va.result() == vals).all()
        rb = red.read_batch()
        assert min(rb.values()) > 0, rb
        return SOME, {"batch": rb}

    under_every_fill(G, monkeypatch, case)


# -------------------------------------------------------------------------------------------------------------- key runs and select


def tile_counts_bytes(tiles, count):
    return (tiles + 1) * 4 if count else 0


@BOTH_WAYS
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4_bytes_on"])
@pytest.mark.parametrize("size", ["0", "T", "3T+5"])
def test_key_runs(G, monkeypatch, size, shift, prepared):
    """No key, a tile, three tiles and five keys; the keys from a 16-byte boundary and 4 bytes behind one, which takes a tile more;
    max_runs below and above the number of runs (two fresh objects a fill)."""
    tile = G.plan_key_runs(1, 32)[0]
    n = {"0": 0, "T": tile, "3T+5": 3 * tile + 5}[size]
    keys = kr.widen(kr.random_runs(np.random.default_rng(70 + n % 97), n), np.uint32)
    R = kr.heads_of(keys, 0xFFFFFFFF).size
    held = tile_counts_bytes(G.plan_key_runs(n, 32)[1], n)

    def case():
        for max_runs in (R // 2, R + 9):
            runs = G.KeyRuns()
            if prepared:
                runs.prepare(n, 32)
            assert kr.check_case(G, runs, keys, max_runs, shift=shift) == R
        return 2 * held, {}

    under_every_fill(G, monkeypatch, case, moves=True if n else False)


@BOTH_WAYS
@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "4_bytes_on"])
@pytest.mark.parametrize("size", ["0", "T", "3T+5"])
def test_select_by_a_byte_stencil(G, monkeypatch, size, shift, prepared):
    """A byte stencil against a threshold, 4-byte items; max_out below and above the number selected."""
    tile = G.plan_select(1, G.SelectStencil_Byte)[0]
    n = {"0": 0, "T": tile, "3T+5": 3 * tile + 5}[size]
    stencil = np.random.default_rng(80 + n % 97).integers(0, 256, n, dtype=np.uint8)
    S = se.selected(stencil, se.GT, 200).size
    held = tile_counts_bytes(G.plan_select(n, G.SelectStencil_Byte)[1], n)

    def case():
        for max_out in (S // 2, S + 9):
            sel = G.Select()
            if prepared:
                sel.prepare(n, G.SelectStencil_Byte)
            assert se.check_case(G, sel, stencil, se.GT, 200, max_out, stencil_shift=shift) == S
        return 2 * held, {}

    under_every_fill(G, monkeypatch, case, moves=True if n else False)


# ------------------------------------------------------------------------------------------------------------------- sorted search


def search_data(key_type, n=40000, m=3000):
    rng = np.random.default_rng(90 + np.dtype(key_type).itemsize)
    if key_type == "uint32":
        hay = ss.sorted_hay(rng, n, np.uint32)
        return hay, ss.needles_for(rng, hay, m, 32)
    hay = np.sort(rng.standard_normal(n) * 1000.0)  # (no NaN and no zero: the numeric order is the sort's)
    hay[::7] = hay[3]
    hay = np.sort(hay)
    return hay, rng.permutation(np.concatenate([rng.standard_normal(m) * 1000.0, hay[rng.integers(0, n, m // 3)], [-np.inf, np.inf]]))


@BOTH_WAYS
@pytest.mark.parametrize("key_type", ["uint32", "float64"])
@pytest.mark.parametrize("path", [ss.DIRECT, ss.INDEXED], ids=["direct", "indexed"])
def test_sorted_search(G, monkeypatch, path, key_type, prepared):
    """Both paths by the option.  The direct search reads no scratch, and an unprepared object of it allocates none."""
    hay, needles = search_data(key_type)
    index_bytes = G.plan_sorted_search(hay.size, needles.size, key_type)[3]
    assert index_bytes > 0

    def case():
        search = G.SortedSearch()
        if prepared:
            search.prepare(hay.size, key_type)
        ss.check_case(G, search, hay, needles, "both", path)  # (last() against the plan: the path that ran)
        return (index_bytes if prepared or path == ss.INDEXED else 0), {"last": search.last()}

    under_every_fill(G, monkeypatch, case, moves=True if prepared or path == ss.INDEXED else None)


@BOTH_WAYS
@pytest.mark.parametrize("key_type", ["uint32", "float64"])
def test_sorted_search_that_reuses_its_index(G, monkeypatch, key_type, prepared):
    """index_ptr, then a search with reuse_index: one kernel each."""
    hay, needles = search_data(key_type)
    levels, index_bytes = G.plan_sorted_search(hay.size, needles.size, key_type)[1], G.plan_sorted_search(hay.size, needles.size, key_type)[3]

    def case():
        search = G.SortedSearch()
        if prepared:
            search.prepare(hay.size, key_type)
        ha = ss.Array(hay)
        search.index_ptr(ha.ptr, hay.size, key_type, ss.stream())
        assert search.last() == (ss.INDEXED, levels, 1)
        ss.check_case(G, search, hay, needles, "both", None, reuse=True, hay_array=ha)
        assert search.last() == (ss.INDEXED, levels, 1)
        return index_bytes, {"last": search.last()}

    under_every_fill(G, monkeypatch, case)


# ------------------------------------------------------------------------------------------------------- merge, set operations, expand

MERGE_KINDS = {"u32keys": ("uint32", False), "u64pairs": ("uint64", True)}


def two_sorted(rng, total, key_type, uniform):
    na = total // 2 + 3
    return uniform(rng, na, key_type), uniform(rng, total - na, key_type)


@BOTH_WAYS
@pytest.mark.parametrize("kind", sorted(MERGE_KINDS))
@pytest.mark.parametrize("size", ["T", "3T+5"])
def test_merge(G, monkeypatch, size, kind, prepared):
    key_type, with_vals = MERGE_KINDS[kind]
    T = mg.tile_of(G, key_type)
    total = T if size == "T" else 3 * T + 5
    a, b = two_sorted(np.random.default_rng(T + total), total, key_type, mg.uniform)
    want = mg.oracle(a, b)
    tiles, kernels, held = G.plan_merge(a.size, b.size, key_type, with_vals)[1:4]
    assert tiles == (1 if size == "T" else 4) and held > 0

    def case():
        merge = G.Merge()
        if prepared:
            merge.prepare(total, key_type)
        mg.check_case(G, merge, a, b, with_vals, want=want)  # (last() against the plan)
        return held, {"last": merge.last()}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("kind", sorted(MERGE_KINDS))
@pytest.mark.parametrize("size", ["T", "3T+5"])
@pytest.mark.parametrize("op", st.OPS + ("count_only",))
def test_set_operations(G, monkeypatch, op, size, kind, prepared):
    """The four operations and the call that only counts (a union without arrays): the bounds, the tile counts and their scan."""
    key_type, with_vals = MERGE_KINDS[kind]
    T = st.tile_of(G, key_type)
    total = T if size == "T" else 3 * T + 5
    below = total // 3  # (duplicates on both sides and across them)
    rng = np.random.default_rng(T + total + 1)
    a, b = st.uniform(rng, total // 2 + 3, key_type, below), st.uniform(rng, total - total // 2 - 3, key_type, below)
    want = st.oracle(a, b)
    count_only = op == "count_only"
    held = G.plan_set_ops(a.size, b.size, key_type, not count_only)[3]
    assert held > 0

    def case():
        sets = G.SetOps()
        if prepared:
            sets.prepare(total, key_type)
        st.check_case(G, sets, "union" if count_only else op, a, b, with_vals, want=want, count_only=count_only)
        return held, {"last": sets.last()}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("size", ["T", "3T+5"])
def test_expand(G, monkeypatch, size, prepared):
    T = ex.tile_of(G)
    M = T if size == "T" else 3 * T + 5  # (the merged sequence: the offsets and the positions)
    n = M // 40
    total = M - n - 1
    lens = ex.split_total(np.random.default_rng(M), total, n)
    lens[::5] = 0
    offsets = ex.offsets_of(lens)
    tiles, kernels, held = G.plan_expand(total, n)[1:4]
    assert tiles == (1 if size == "T" else 4) and held > 0

    def case():
        expand = G.Expand()
        if prepared:
            expand.prepare(total, n)
        ex.check_case(G, expand, offsets, total)
        return held, {"last": expand.last()}

    under_every_fill(G, monkeypatch, case)


def test_expand_from_counts(G, monkeypatch):
    """The counts form, the header's recipe: a fresh BlellochScan turns counts[0 .. n] into offsets in place by the one-segment
    exclusive scan, a fresh Expand takes them from there."""
    import torch

    T = ex.tile_of(G)
    n = 3 * T // 40
    lens = np.random.default_rng(5).integers(0, 70, n)
    total = int(lens.sum())
    want = ex.offsets_of(lens)

    def case():
        scan, expand = G.BlellochScan(G.DataType_Uint), G.Expand()
        counts = torch.from_numpy(np.concatenate([lens, [12345]]).astype(np.uint32).view(np.int32)).cuda()
        sb.sync()
        scan.run_whole_ptr(counts.data_ptr(), n + 1, ex.stream())
        sb.sync()
        offsets = counts.cpu().numpy().view(np.uint32)
        assert (offsets == want).all()
        ex.check_case(G, expand, offsets, total)
        return G.plan_expand(total, n)[3], {"last": expand.last(), "batch": scan.read_batch()}

    under_every_fill(G, monkeypatch, case)


# ----------------------------------------------------------------------------------------------------------------------- histogram


@BOTH_WAYS
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("bins", [256, 8192, 8193])
def test_histogram_of_even_bins(G, monkeypatch, bins, accumulate, prepared):
    """Three tiles and a few samples over 256 and 8192 bins (a row of `partial` per workgroup, summed by a second kernel) and over 8193,
    where the counts are added straight to the caller's array and the object needs no scratch."""
    tile = hi.tile_and_groups_max(G, "uint32", "even")[0]
    n = 3 * tile + 77
    rng = np.random.default_rng(bins)
    lo, hi_ = 1000, 1000 + 7 * bins
    x = hi.samples_of(rng, n, "uint32", lo, hi_)
    prior = rng.integers(0, 2**32, bins, dtype=np.uint32) if accumulate else None
    path, _, _, groups, _, held = G.plan_histogram(n, bins, "uint32", "even")
    assert path == (hi.LDS if bins <= 8192 else hi.GLOBAL) and (groups >= 3 and held > 0 if path == hi.LDS else held == 0)

    def case():
        h = G.Histogram()
        if prepared:
            h.prepare(n, bins)
        hi.check_even(G, h, x, lo, hi_, bins, prior=prior)  # (last() against the plan: the path)
        return held, {"last": h.last()}

    under_every_fill(G, monkeypatch, case, moves=True if held else None)


@BOTH_WAYS
def test_histogram_of_uint64_edges(G, monkeypatch, prepared):
    tile = hi.tile_and_groups_max(G, "uint64", "edges")[0]
    n, bins = 3 * tile + 77, 300
    rng = np.random.default_rng(7)
    x = hi.samples_of(rng, n, "uint64", 1000, 2**40)
    e = hb.edges_of(rng, "uint64", bins, 1000, 2**40)
    x[:e.size] = e
    held = G.plan_histogram(n, bins, "uint64", "edges")[5]
    assert held > 0

    def case():
        h = G.Histogram()
        if prepared:
            h.prepare(n, bins)
        hi.check_edges(G, h, x, e)
        return held, {"last": h.last()}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("mode", ["even", "edges"])
def test_batched_histogram(G, monkeypatch, mode, prepared):
    """One batch with a segment of each class, the long one of three chunks, and empty segments (`batch_lists`, `batch_partial`)."""
    bins = 640
    wave_limit, block_limit, chunk = hb.limits(G, bins, "uint32", mode)
    lens = np.array([0, 7, wave_limit, block_limit, 2 * chunk + 1, 0, 0])
    classes = hb.classes_of(G, lens, bins, "uint32", mode)
    assert classes == {"wave": 2, "block": 1, "long": 1}
    rng = np.random.default_rng(len(mode))
    x = hb.samples_of(rng, int(lens.sum()), "uint32", 1000, 1000 + 7 * bins)
    offsets = hb.offsets_of(lens)
    kw = dict(even=(1000, 1000 + 7 * bins)) if mode == "even" else dict(edges=hb.edges_of(rng, "uint32", bins, 1000, 1000 + 7 * bins))

    def case():
        h = G.Histogram()
        if prepared:
            h.prepare_batch(x.size, lens.size, bins)
        hb.check_batch(G, h, x, offsets, bins, **kw)  # (last() and read_batch() against the plan)
        return SOME, {"last": h.last(), "batch": h.read_batch()}

    under_every_fill(G, monkeypatch, case)


# --------------------------------------------------------------------------------------------------------------------------- top-k

TOP_K_N, TOP_K_K = 300001, 100


def top_k_keys(kind):
    rng = np.random.default_rng(100 + len(kind))
    if kind == "float32_one_exponent":  # every key in [1, 2): round 0's digit is one value, no bucket of it fits
        return (1.0 + rng.random(TOP_K_N)).astype(np.float32)
    return tk.random_keys(rng, kind, TOP_K_N)


TOP_K_CASES = {  # keys, PATH, CAND_CAPACITY, largest, sorted, the path the case is meant to take (None: as the bucket falls)
    "auto_sorted": ("uint32", tk.AUTO, 0, False, True, tk.CANDIDATES),
    "auto_unsorted": ("uint32", tk.AUTO, 0, True, False, tk.CANDIDATES),
    "full_sorted": ("uint32", tk.FULL, 0, True, True, tk.FULL),
    "full_unsorted": ("uint32", tk.FULL, 0, False, False, tk.FULL),
    "uint64_six_rounds": ("uint64", tk.AUTO, 0, False, True, tk.CANDIDATES),
    "one_exponent": ("float32_one_exponent", tk.AUTO, 0, False, True, None),
    "bucket_does_not_fit": ("uint32", tk.AUTO, 64, False, True, tk.FULL),
}


def top_k_path(keys, k, largest, option, plan):
    """The path the header's rule gives: FULL by the option, or where the bucket of round 0's crossing digit holds more code words than
    the candidate buffer (plan["capacity"]); the digit is plan["digits"][0]."""
    shift, bits = plan["digits"][0]
    code = key_code(keys, largest)
    counts = np.bincount((code >> code.dtype.type(shift)).astype(np.int64) & ((1 << bits) - 1), minlength=1 << bits)
    bucket = int(counts[np.searchsorted(np.cumsum(counts), k)])
    return tk.FULL if option == tk.FULL or bucket > plan["capacity"] else tk.CANDIDATES


@BOTH_WAYS
@pytest.mark.parametrize("name", sorted(TOP_K_CASES))
def test_top_k(G, monkeypatch, name, prepared):
    """300 001 keys, k = 100: round 0 (`state`, `partial`), the candidates (`cand`) or the input again for every round, the two count
    scans, the ordering (`pairs`) -- then read_last, the struct copied back from `state`."""
    kind, path, capacity, largest, sorted_, reported = TOP_K_CASES[name]
    keys = top_k_keys(kind)
    name_of = keys.dtype.name
    plan = G.plan_top_k(TOP_K_N, TOP_K_K, name_of, sorted=sorted_, path=path, cand_capacity=capacity)
    assert name_of != "uint64" or plan["rounds"] == 6
    want_path = top_k_path(keys, TOP_K_K, largest, path, plan)
    assert reported in (None, want_path), (name, want_path)
    # (the plan counts the pairs of the ordering, which an unsorted call does not reserve and a prepare does)
    held = plan["scratch_bytes"] - (0 if sorted_ or prepared else TOP_K_K * (keys.dtype.itemsize + 4))

    def case():
        top = tk.with_options(G, path, capacity)
        if prepared:
            top.prepare(TOP_K_N, TOP_K_K, name_of)
        last = tk.check_case(G, top, keys, TOP_K_K, largest, sorted_)
        assert last["path"] == want_path, last
        return held, {"last": last}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
def test_batched_top_k_of_offsets(G, monkeypatch, sorted_, prepared):
    """Wave, block and long segments and two empty ones in one batch (`batch_lists`); sorted: the rows of pairs (`batch_rows`), of which
    those of the empty segments are never written, ordered in place by the batched sort and skipped by the decode kernel."""
    limits = G.plan_top_k_batch(1, 1, 1, "uint32")["limits"]
    lens = [0, 100, limits[0], limits[1], limits[3], limits[3] + 1000, 0, 9]
    offsets = tkb.offsets_of(lens, 3)
    keys = tk.random_keys(np.random.default_rng(110), "uint32", int(offsets[-1]) + 5)
    classes = tkb.classes_of(G, tkb.clamp_segments(offsets, keys.size), "uint32")
    assert min(classes.values()) > 0
    k = 40

    def case():
        top = G.TopK()
        if prepared:
            top.prepare_batch(keys.size, len(lens), k, "uint32")
        last, plan = tkb.run_case(G, top, keys, k, False, sorted_, offsets=offsets)
        assert {c: last[c] for c in classes} == classes, last
        return plan["scratch_bytes"], {"batch": last}

    under_every_fill(G, monkeypatch, case)


@BOTH_WAYS
def test_batched_top_k_on_the_loop_path(G, monkeypatch, prepared):
    """Equal partitions at BATCH_LOOP_MIN, set to their length: the single call partition after partition."""
    limits = G.plan_top_k_batch(1, 1, 1, "uint32")["limits"]
    n, parts, k = limits[3] + 1000, 3, 77
    keys = tk.random_keys(np.random.default_rng(111), "uint32", parts * n)

    def case():
        top = G.TopK({"BATCH_LOOP_MIN": n})
        if prepared:
            top.prepare_batch(parts * n, parts, k, "uint32")
        last, plan = tkb.run_case(G, top, keys, k, True, True, count=n, parts=parts, loop_min=n)
        assert plan["path"] == G.TopKBatch_Loop and last["long"] == parts, (plan, last)
        return plan["scratch_bytes"], {"batch": last}

    under_every_fill(G, monkeypatch, case)


# -------------------------------------------------------------------------------------------------------------------- sharded sort


def _sharded_worker(q):
    """Own process, as test_gpu_dist.py runs the world of one with the repartition forced: a fresh Dist a fill, one sort of 13-bit
    keys each."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "gl-radix-sort_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["GLU_HIP_DIST_TEST_REPARTITION"] = "1"
    import ctypes

    import torch
    import glu_hip as g
    import oracle as o

    torch.cuda.set_device(0)
    g.set_device(0)
    n = 700001
    keys = (np.random.default_rng(13).integers(0, 2**32, n, dtype=np.uint64) & ((1 << 13) - 1)).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    ek, ev = o.stable_sort_pairs(keys, vals)

    def read_back(ptr):  # (the shard lives in the library's own arrays)
        h = ctypes.c_uint32(0)
        g.check(g.lib().glu_buffer_wrap(ctypes.c_void_p(ptr), n * 4, ctypes.byref(h)))
        host = np.empty(n, dtype=np.uint32)
        g.check(g.lib().glu_buffer_read(h, host.ctypes.data_as(ctypes.c_void_p), n * 4, 0))
        g.check(g.lib().glu_buffer_destroy(h))
        return host

    out = []
    for fill in FILLS:
        os.environ[ENV] = str(fill)
        before = g.scratch_filled_bytes()
        d = g.Dist(g.dist_unique_id(), 1, 0)
        kt, vt = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            kp, vp, cnt = d.sort_ptr(kt.data_ptr(), vt.data_ptr(), n, stream.cuda_stream)
        stream.synchronize()
        ok = cnt == n and bool((read_back(kp) == ek).all()) and bool((read_back(vp) == ev).all())
        out.append((ok, d.partition_shift(), d.last_local_sort(), d.last_rounds(), d.sorter.scratch_size(), g.scratch_filled_bytes() - before))
        d.destroy()
    q.put(out)


def test_sharded_sort_of_one_rank_with_the_repartition(built):
    """The world of one with the lower-byte fallback forced, in a process of its own (a communicator wants the process's device): the
    shard against the oracle, the partition byte, and the counter beyond the local sorter's own scratch."""
    import queue

    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_sharded_worker, args=(q,))
    p.start()
    try:
        out = q.get(timeout=120)
    except queue.Empty:
        p.join(timeout=5)
        raise AssertionError("the worker produced nothing (exit code %s)" % p.exitcode)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert len(out) == len(FILLS)
    for fill, (ok, shift, local_sort, rounds, sorter_bytes, grew) in zip(FILLS, out):
        assert ok and shift == 8, (fill, out)
        assert grew > sorter_bytes > 0, (fill, out)  # (the send and the receive pair and the histogram rows on top of the sorter's)
        assert (shift, local_sort, rounds, sorter_bytes) == out[0][1:5], (fill, out)


# --------------------------------------------------------------------------------------------------- the operators without scratch


def test_gather_and_scatter_fill_nothing(G, monkeypatch):
    """Gather owns no device memory: one gather and one scatter of three tiles and five entries, and the counter does not move."""
    item_bytes = 16
    n = 3 * ga.tile_of(G, item_bytes) + 5
    rng = np.random.default_rng(120)
    items, idx = ga.records(rng, n, item_bytes), rng.permutation(n).astype(np.uint32)

    def case():
        g = G.Gather()
        ga.check_gather(G, g, items, idx)
        told = {"gather": g.last()}
        ga.check_scatter(G, g, items, idx, n)
        told["scatter"] = g.last()
        return 0, told

    under_every_fill(G, monkeypatch, case, moves=False)


def test_batched_sorted_search_fills_nothing(G, monkeypatch):
    """37 rows of 100 needles in rows of 128 keys: one kernel on a fresh object, no scratch."""
    P, n, m = 37, 128, 100
    rng = np.random.default_rng(121)
    hay = ssb.sorted_rows(rng, np.arange(P + 1) * n, 300, "uint32")
    needles = ssb.keys_of(rng.integers(0, 302, P * m), "uint32")

    def case():
        search = G.SortedSearch()
        ssb.check_batch(G, search, hay, needles, rows=(P, n, m))
        return 0, {"last": search.last()}

    under_every_fill(G, monkeypatch, case, moves=False)
