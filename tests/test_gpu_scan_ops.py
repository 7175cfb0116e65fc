"""GPU tests of the batched scan with an operator and a kind (glu_scan_run_batch_offsets_op_ptr): Sum, Mul, Min, Max, exclusive or
inclusive, in place or into a second array, per segment, by key, and over a whole array without offsets.  Inputs and expected
values are scan_ops_cases.py's (exact in any grouping, so `==` is the check; tests/test_scan_ops_cases.py proves that without a
GPU); floats that do round have tests of their own against exact arithmetic.  Every array lies between guards of poison inside
its allocation and the whole allocation is compared.  Class limits come from plan_scan_batch."""
import ctypes
import gc

import numpy as np
import pytest

import scan_ops_cases as sc

pytestmark = pytest.mark.gpu
GUARD = 8  # elements of poison in front of and behind an array, inside its allocation
KINDS = (False, True)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def last_where(pred, hi=1 << 40):
    lo = 0  # pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def class_limits(G, es):
    """Last length of the wave class, last length of the workgroup class, the chunk of the long class (from plan_scan_batch) and
    the tile of the workgroup's loop: 256 threads x 4 groups x one 16-byte pack, so half a chunk of 32 KiB, or a whole one for
    the 32-byte type, whose pack is one element."""
    wave = last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 1)
    block = last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 2)
    w0 = G.plan_scan_batch(block + 1, es)[1]
    chunk = last_where(lambda c: c <= block or G.plan_scan_batch(c, es)[1] <= w0) // w0
    assert G.plan_scan_batch(wave + 1, es)[0] == 2 and G.plan_scan_batch(block + 1, es)[0] == 3
    assert G.plan_scan_batch(3 * chunk + 1, es) == (3, 4)
    tile = chunk // 2 if es < 32 else chunk
    return wave, block, chunk, tile


def poison_of(npdt):
    """A pattern no scan of the drawn inputs produces: a NaN with a payload for floats, a fixed even word for integers."""
    if npdt == np.float32:
        return np.array([0x7FC5A5A5], dtype=np.uint32).view(np.float32)[0]
    if npdt == np.float64:
        return np.array([0x7FF8A5A5A5A5A5A5], dtype=np.uint64).view(np.float64)[0]
    return np.array([0xA5A5A5A4], dtype=np.uint32).view(npdt)[0]


class Array:
    """`d` on the device, `shift` elements behind a 16-byte boundary, poison in front of and behind it inside the allocation."""

    def __init__(self, d, dt, shift=0):
        import torch

        npdt, comps = sc.dtype_info(dt)
        self.npdt, self.comps, self.es = npdt, comps, npdt().itemsize * comps
        self.front = (GUARD + shift) * comps
        self.host = np.concatenate([np.full(self.front, poison_of(npdt), dtype=npdt), d, np.full(GUARD * comps, poison_of(npdt), dtype=npdt)])
        self.n = d.size // comps
        self.t = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0 and (GUARD * self.es) % 16 == 0
        self.ptr = self.t.data_ptr() + (GUARD + shift) * self.es

    def result(self):
        """The array after the call; asserts that the poison around it is intact."""
        raw = self.t.cpu().numpy()
        want = self.host.view(np.uint8)
        lo, hi = self.front * self.npdt().itemsize, (self.front + self.n * self.comps) * self.npdt().itemsize
        assert (raw[:lo] == want[:lo]).all() and (raw[hi:] == want[hi:]).all(), "the call wrote outside the array"
        return raw[lo:hi].copy().view(self.npdt)


def poison_array(dt, total, shift=0):
    npdt, comps = sc.dtype_info(dt)
    return Array(np.full(total * comps, poison_of(npdt), dtype=npdt), dt, shift)


def device_offsets(offsets):
    import torch

    return torch.from_numpy(np.asarray(offsets, dtype=np.uint32).view(np.int32).copy()).cuda()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def scan_call(G, scan, d, dt, offsets, op, inclusive, out_of_place, shift=0, out_shift=0, whole=False):
    """One call on fresh arrays.  Returns (what the results were stored to, data after the call): the same array in place."""
    import torch

    data = Array(d, dt, shift)
    out = poison_array(dt, data.n, out_shift) if out_of_place else None
    ot = None if whole else device_offsets(offsets)
    if whole:
        scan.run_whole_ptr(data.ptr, data.n, stream(), out_ptr=out.ptr if out else None, op=op, inclusive=inclusive)
    else:
        scan.run_batch_offsets_ptr(data.ptr, data.n, ot.data_ptr(), len(offsets) - 1, stream(), out_ptr=out.ptr if out else None, op=op,
                                   inclusive=inclusive)
    torch.cuda.synchronize()
    after = data.result()
    return (out.result() if out else after), after


def poison_like(d):
    return np.full_like(d, poison_of(d.dtype.type))


# ---------------------------------------------------------------------------------------------------- all types and classes


@pytest.mark.parametrize("dt", range(12))
def test_every_type_operator_and_kind_across_the_class_boundaries(G, dt):
    """One batch per type: the lengths at which a kernel takes another path, two empty segments between each two of them, a head
    and a tail of the array outside the segments.  Four operators x two kinds, in place and into an array of poison: outside the
    segments `out` keeps its poison and in place the data its values; `data` is unchanged when `out` is given."""
    npdt, comps = sc.dtype_info(dt)
    es = npdt().itemsize * comps
    wave, block, chunk, tile = class_limits(G, es)
    lens = sc.with_empty_between(sc.boundary_lengths(wave, block, chunk, tile))
    head, tail = 5, 3
    offsets = np.concatenate([[0], np.cumsum(lens)]) + head
    total = int(offsets[-1]) + tail
    scan = G.BlellochScan(dt)
    paths = [G.plan_scan_batch(n, es)[0] for n in lens]
    assert min(paths.count(p) for p in (1, 2, 3)) > 0
    for op in sc.OPS:
        d = sc.make_data(np.random.default_rng(100 * dt + sc.OPS.index(op)), dt, op, offsets, total)
        for inclusive in KINDS:
            for out_of_place in (False, True):
                got, after = scan_call(G, scan, d, dt, offsets, op, inclusive, out_of_place)
                want = sc.expected(d, dt, op, inclusive, offsets, base=poison_like(d) if out_of_place else None)
                where = (op, inclusive, out_of_place)
                assert sc.same(op, npdt, got, want), (where, sc.first_difference(got, want, comps))
                if out_of_place:
                    assert sc.same_bits(after, d), (where, "data changed")
                rb = scan.read_batch()
                assert [rb["wave"], rb["block"], rb["long"]] == [paths.count(p) for p in (1, 2, 3)], where


# ------------------------------------------------------------------------------------------------------------ address shifts


def rounding_values(rng, op, npdt, n):
    """Values whose scans do round: the bits show any change in the order of combination."""
    if op == "mul":
        return rng.uniform(0.999, 1.001, n).astype(npdt)
    return rng.standard_normal(n).astype(npdt)


@pytest.mark.parametrize("dt,op", [(0, "sum"), (0, "mul"), (3, "max"), (2, "min"), (3, "sum")])
def test_the_store_side_never_changes_the_bits(G, dt, op):
    """4-byte types, `data` 0 .. 3 elements behind a 16-byte boundary: `out` at the same shift (16-byte stores) and at a different
    one (single elements) give the same bits as each other and as the call in place, for segments of every class that start at
    every address modulo 16.  Floats are values that round."""
    npdt, comps = sc.dtype_info(dt)
    wave, block, chunk, tile = class_limits(G, 4)
    rng = np.random.default_rng(300 + dt)
    lens = []
    for n in (1, 2, 3, 5, 33, 200, wave, wave + 1, tile + 1, block, block + 1, 2 * chunk + 3):
        lens += [n, int(rng.integers(0, 4))]
    lens += [9, 1, 11, 2, 13]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    assert {int(b) % 4 for b in offsets[:-1]} == {0, 1, 2, 3}
    total = int(offsets[-1])
    d = rounding_values(rng, op, npdt, total) if sc.is_float(npdt) else sc.make_data(rng, dt, op, offsets, total)
    scan = G.BlellochScan(dt)
    for shift in range(4):
        in_place, _ = scan_call(G, scan, d, dt, offsets, op, True, False, shift=shift)
        if not sc.is_float(npdt):
            assert sc.same_bits(in_place, sc.expected(d, dt, op, True, offsets)), shift
        for out_shift in (shift, (shift + 1) % 4, (shift + 2) % 4):
            got, after = scan_call(G, scan, d, dt, offsets, op, True, True, shift=shift, out_shift=out_shift)
            assert sc.same_bits(after, d)
            assert sc.same_bits(got, in_place), (shift, out_shift, sc.first_difference(got, in_place, 1))


# ------------------------------------------------------------------------------------------- partials over several tiles


@pytest.mark.parametrize("op,inclusive", [("max", True), ("mul", False)])
def test_a_long_segment_whose_partials_take_two_tiles_of_their_scan(G, op, inclusive):
    """dvec4, 32 bytes, the cheapest: a chunk is 1024 elements and a tile of the partials' scan 1024 partials, so 1024 chunks and
    one element (2^20 + 1 elements, 32 MiB) need a second tile.  Out of place."""
    dt = 7
    npdt, comps = sc.dtype_info(dt)
    wave, block, chunk, tile = class_limits(G, 32)
    n = tile * chunk + 1
    assert n <= 1 << 21 and G.plan_scan_batch(n, 32) == (3, tile + 1)
    offsets = [2, 2 + n]
    d = sc.make_data(np.random.default_rng(7), dt, op, offsets, n + 4)
    scan = G.BlellochScan(dt)
    got, after = scan_call(G, scan, d, dt, offsets, op, inclusive, True)
    want = sc.expected(d, dt, op, inclusive, offsets, base=poison_like(d))
    assert sc.same(op, npdt, got, want), sc.first_difference(got, want, comps)
    assert sc.same_bits(after, d)
    assert scan.read_batch() == {"wave": 0, "block": 0, "long": 1}


# ------------------------------------------------------------------------------------------------------- order of binning


def test_float_products_do_not_depend_on_the_order_of_binning(G):
    """Inclusive float32 Mul on values that round (uniform in [0.999, 1.001]): three long segments of 3, 5 and 9 chunks, more
    than 256 segments apart, so that their chunk slots -- and the alignment of their runs of partials -- follow the order in
    which workgroups of the binning kernel arrive.  Each comes out bit for bit as when it is scanned alone, and the whole call
    gives the same bits twice."""
    dt, op = 0, "mul"
    wave, block, chunk, tile = class_limits(G, 4)
    rng = np.random.default_rng(16)
    lens = rng.integers(0, 40, 900)
    long_at = {10: 3, 400: 5, 800: 9}
    for s, chunks in long_at.items():
        lens[s] = chunks * chunk - 7
        assert G.plan_scan_batch(int(lens[s]), 4) == (3, chunks)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = rounding_values(rng, op, np.float32, int(offsets[-1]))
    scan = G.BlellochScan(dt)
    first, _ = scan_call(G, scan, d, dt, offsets, op, True, True)
    assert scan.read_batch()["long"] == 3
    second, _ = scan_call(G, scan, d, dt, offsets, op, True, True)
    assert sc.same_bits(first, second), "the same call gave different bits"
    for s in long_at:
        b, e = int(offsets[s]), int(offsets[s + 1])
        alone, _ = scan_call(G, scan, d, dt, [b, e], op, True, True)
        assert scan.read_batch() == {"wave": 0, "block": 0, "long": 1}
        assert sc.same_bits(alone[b:e], first[b:e]), (s, sc.first_difference(alone[b:e], first[b:e], 1))
        assert sc.same_bits(alone[:b], poison_like(d)[:b]) and sc.same_bits(alone[e:], poison_like(d)[e:])


# ---------------------------------------------------------------------------------------------------------------- rounding


def as_integer_times_power(v):
    """(m, e) with v == m * 2^e exactly, m an integer."""
    num, den = float(v).as_integer_ratio()
    return (num, -(den.bit_length() - 1))


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("op", ["sum", "mul"])
def test_floats_that_round_stay_inside_the_bounds_of_any_grouping(G, dt, op):
    """float32 / float64, one medium and one long segment, inclusive, against exact integer arithmetic (every float is an integer
    times a power of two).  Element i, the result over n = i + 1 values:
      Sum  |got - exact| <= n u sum_{j <= i} |x_j|
      Mul  |got - exact| <= n u / (1 - n u) |exact|
    with u = 2^-24 / 2^-53: the standard bounds of a sum and a product in ANY grouping (Higham, Accuracy and Stability of
    Numerical Algorithms, sections 4.2 and 3.4); nothing measured enters them."""
    npdt, _ = sc.dtype_info(dt)
    es = npdt().itemsize
    wave, block, chunk, tile = class_limits(G, es)
    lens = [wave + 7, block + 11]
    assert [G.plan_scan_batch(n, es)[0] for n in lens] == [2, 3]
    offsets = np.concatenate([[1], 1 + np.cumsum(lens)])
    rng = np.random.default_rng(400 + dt)
    d = rounding_values(rng, op, npdt, int(offsets[-1]) + 1)
    ubits = 24 if dt == 0 else 53
    got, _ = scan_call(G, G.BlellochScan(dt), d, dt, offsets, op, True, True)
    for b, e in zip(offsets[:-1], offsets[1:]):
        worst = 0.0
        if op == "sum":
            # everything in units of 2^-1200: integers
            scale = 1200
            acc = abs_sum = 0
            for i, (x, g) in enumerate(zip(d[b:e].tolist(), got[b:e].tolist())):
                m, ex = as_integer_times_power(x)
                acc += m << (ex + scale)
                abs_sum += abs(m) << (ex + scale)
                gm, ge = as_integer_times_power(g)
                err = abs((gm << (ge + scale)) - acc)
                # err <= n * 2^-ubits * abs_sum
                assert (err << ubits) <= (i + 1) * abs_sum, (int(e - b), i, g)
                if abs_sum:
                    worst = max(worst, (err << ubits) / ((i + 1) * abs_sum))
        else:
            acc_m, acc_e = 1, 0
            for i, (x, g) in enumerate(zip(d[b:e].tolist(), got[b:e].tolist())):
                m, ex = as_integer_times_power(x)
                acc_m, acc_e = acc_m * m, acc_e + ex
                gm, ge = as_integer_times_power(g)
                # |gm 2^ge - acc_m 2^acc_e| (2^ubits - n) <= n |acc_m| 2^acc_e, both sides in units of 2^min(ge, acc_e)
                low = min(ge, acc_e)
                err = abs((gm << (ge - low)) - (acc_m << (acc_e - low)))
                n = i + 1
                assert err * ((1 << ubits) - n) <= n * (abs(acc_m) << (acc_e - low)), (int(e - b), i, g)
        print("%s %s n = %d: inside the bound%s" % (npdt.__name__, op, e - b, ", largest error / bound = %.3g" % worst if op == "sum" else ""))


# -------------------------------------------------------------------------------------------------------- one-segment form


@pytest.mark.parametrize("dt,op,inclusive", [(3, "sum", True), (0, "max", True), (1, "mul", False), (9, "min", True)])
def test_null_offsets_scan_the_whole_array(G, dt, op, inclusive):
    """offsets == NULL, one segment: total = 1, the workgroup limit + 1 and 3 chunks + 1.  Equal to the call with the explicit
    offsets [0, total] bit for bit, and to the expected values; in place and out of place."""
    npdt, comps = sc.dtype_info(dt)
    es = npdt().itemsize * comps
    wave, block, chunk, tile = class_limits(G, es)
    scan = G.BlellochScan(dt)
    for total in (1, block + 1, 3 * chunk + 1):
        offsets = [0, total]
        d = sc.make_data(np.random.default_rng(total), dt, op, offsets, total)
        for out_of_place in (False, True):
            got, after = scan_call(G, scan, d, dt, None, op, inclusive, out_of_place, whole=True)
            rb = scan.read_batch()
            assert rb["wave"] + rb["block"] + rb["long"] == 1
            explicit, _ = scan_call(G, scan, d, dt, offsets, op, inclusive, out_of_place)
            assert sc.same_bits(got, explicit), (total, out_of_place)
            want = sc.expected(d, dt, op, inclusive, offsets)
            assert sc.same(op, npdt, got, want), (total, out_of_place, sc.first_difference(got, want, comps))
            if out_of_place:
                assert sc.same_bits(after, d)


# ------------------------------------------------------------------------------------------------------------------ by key


def running_maximum_by_key(G, scan, runs):
    """run_by_key_ptr with op="max", inclusive=True and an `out` array on `scan` (of uint32) and `runs`, objects made by the caller, on
    sorted keys with runs of every class, against numpy.  Returns (out, read_batch)."""
    import torch

    dt, op = 3, "max"
    wave, block, chunk, tile = class_limits(G, 4)
    rng = np.random.default_rng(21)
    lens = [1, 2, 30, wave, wave + 1, 3000, block, block + 1, 2 * chunk + 5, 7]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    count = int(offsets[-1])
    keys = np.repeat(np.sort(rng.choice(1 << 20, len(lens), replace=False)).astype(np.uint32), lens)
    d = sc.make_data(rng, dt, op, offsets, count)
    max_runs = len(lens) + 5
    kt = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    ot = torch.zeros(max_runs + 1, dtype=torch.int32, device="cuda")
    nt = torch.zeros(1, dtype=torch.int32, device="cuda")
    data, out = Array(d, dt), poison_array(dt, count)
    scan.run_by_key_ptr(runs, kt.data_ptr(), data.ptr, count, ot.data_ptr(), max_runs, nt.data_ptr(), stream=stream(), out_ptr=out.ptr, op=op,
                        inclusive=True)
    torch.cuda.synchronize()
    assert int(nt.cpu()[0]) == len(lens)
    assert (ot.cpu().numpy().view(np.uint32)[:len(lens) + 1] == offsets).all()
    want = np.concatenate([np.maximum.accumulate(d[b:e]) for b, e in zip(offsets[:-1], offsets[1:])])
    assert sc.same_bits(out.result(), want)
    assert sc.same_bits(data.result(), d)
    rb = scan.read_batch()
    assert rb["wave"] > 0 and rb["block"] > 0 and rb["long"] > 0
    return out.result(), rb


def test_running_maximum_by_key(G):
    """run_by_key_ptr with op="max", inclusive=True and an `out` array, on sorted keys with runs of every class, against numpy."""
    running_maximum_by_key(G, G.BlellochScan(3), G.KeyRuns())


# ------------------------------------------------------------------------------------------------------------ graph capture


def test_a_captured_out_of_place_inclusive_sum_replays_on_new_inputs(G):
    """After prepare_batch: one out-of-place inclusive Sum over a mixed batch captured on a side stream (a linear graph: the
    call enqueues on the one stream it is given) and replayed twice, each time on another input copied into the captured `data`;
    both results are exact and the data is as it was copied."""
    import torch

    dt, op = 3, "sum"
    wave, block, chunk, tile = class_limits(G, 4)
    rng = np.random.default_rng(31)
    lens = np.concatenate([rng.integers(0, 70, 300), [wave, wave + 1, block, block + 1, 3 * chunk + 1, 0, 0, 2 * chunk + 9]])
    rng.shuffle(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total, nseg = int(offsets[-1]), lens.size
    scan = G.BlellochScan(dt)
    dt_ = torch.zeros(total, dtype=torch.int32, device="cuda")
    out = torch.zeros(total, dtype=torch.int32, device="cuda")
    ot = device_offsets(offsets)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def call(s):
        scan.run_batch_offsets_ptr(dt_.data_ptr(), total, ot.data_ptr(), nseg, s, out_ptr=out.data_ptr(), op=op, inclusive=True)

    with torch.cuda.stream(side):
        scan.prepare_batch(total, nseg)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            d = sc.make_data(rng, dt, op, offsets, total)
            dt_.copy_(torch.from_numpy(d.view(np.int32)))
            out.fill_(-1)
            graph.replay()
            side.synchronize()
            assert sc.same_bits(out.cpu().numpy().view(np.uint32), sc.expected(d, dt, op, True, offsets)), rep
            assert sc.same_bits(dt_.cpu().numpy().view(np.uint32), d), rep


# ----------------------------------------------------------------------------------------------------------------- refusals


def test_refusals_leave_the_arrays_untouched(G):
    import torch

    dt = 3
    n = 1000
    d = np.arange(n, dtype=np.uint32)
    data, out = Array(d, dt), poison_array(dt, n)
    ot = device_offsets([0, 10, n])
    scan = G.BlellochScan(dt)
    L, vp = G.lib(), ctypes.c_void_p
    fp = ot.data_ptr()

    def raw(data_ptr, out_ptr, offsets_ptr, nseg, op, kind):
        G.check(L.glu_scan_run_batch_offsets_op_ptr(scan._h, vp(data_ptr), vp(out_ptr), n, vp(offsets_ptr), nseg, op, kind, None))

    bad = [
        (lambda: raw(data.ptr, out.ptr, fp, 2, 4, 0), "Invalid reduce operator"),
        (lambda: raw(data.ptr, out.ptr, fp, 2, -1, 1), "Invalid reduce operator"),
        (lambda: raw(data.ptr, out.ptr, fp, 2, 0, 2), "Invalid scan kind"),
        (lambda: raw(data.ptr, out.ptr, None, 2, 3, 1), "NULL offsets mean one segment"),
        (lambda: raw(data.ptr, data.ptr + 4, fp, 2, 0, 1), "out overlaps data"),
        (lambda: raw(data.ptr + 4 * (n - 1), data.ptr, fp, 2, 0, 1), "out overlaps data"),
        (lambda: raw(data.ptr, out.ptr + 2, fp, 2, 0, 1), "out is not aligned"),
        (lambda: raw(data.ptr + 2, out.ptr, fp, 2, 0, 1), "data is not aligned"),
        (lambda: raw(None, out.ptr, fp, 2, 0, 1), "Invalid data buffer"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert sc.same_bits(data.result(), d) and sc.same_bits(out.result(), poison_like(d))
    # adjacent arrays do not overlap, and NULL offsets with no segment at all are nothing to do
    wide = Array(np.arange(2 * n, dtype=np.uint32), dt)
    G.check(L.glu_scan_run_batch_offsets_op_ptr(scan._h, vp(wide.ptr), vp(wide.ptr + 4 * n), n, vp(fp), 2, 0, 1, None))
    G.check(L.glu_scan_run_batch_offsets_op_ptr(scan._h, None, None, 0, None, 0, 0, 1, None))
    torch.cuda.synchronize()
    got = wide.result()
    assert sc.same_bits(got[:n], np.arange(n, dtype=np.uint32))
    assert sc.same_bits(got[n:], sc.expected(np.arange(n, dtype=np.uint32), dt, "sum", True, [0, 10, n]))


# ------------------------------------------------------------------------------------------------- old entry point unchanged


def test_the_old_entry_point_and_the_new_one_agree_bit_for_bit(G):
    """glu_scan_run_batch_offsets_ptr, and op = Sum, kind = EXCLUSIVE, out = NULL (and out = data) of the new call: identical
    bytes on a mixed float32 batch of values that round; the same exclusive Sum out of place has the same bits too."""
    import torch

    dt = 0
    wave, block, chunk, tile = class_limits(G, 4)
    rng = np.random.default_rng(41)
    lens = np.concatenate([rng.integers(0, 600, 200), [wave, wave + 1, tile + 3, block, block + 1, 3 * chunk + 1, 5 * chunk - 9]])
    rng.shuffle(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total, nseg = int(offsets[-1]), lens.size
    d = rng.standard_normal(total).astype(np.float32)
    scan = G.BlellochScan(dt)
    ot = device_offsets(offsets)
    L, vp = G.lib(), ctypes.c_void_p
    results = []
    for form in ("old", "new_null", "new_same"):
        arr = Array(d, dt, shift=1)
        if form == "old":
            G.check(L.glu_scan_run_batch_offsets_ptr(scan._h, vp(arr.ptr), total, vp(ot.data_ptr()), nseg, vp(stream())))
        else:
            G.check(L.glu_scan_run_batch_offsets_op_ptr(scan._h, vp(arr.ptr), vp(arr.ptr) if form == "new_same" else None, total,
                                                        vp(ot.data_ptr()), nseg, 0, 0, vp(stream())))
        torch.cuda.synchronize()
        results.append(arr.result())
    assert sc.same_bits(results[0], results[1]) and sc.same_bits(results[0], results[2])
    assert results[0][int(offsets[np.argmax(lens)])] == 0 and not sc.same_bits(results[0], d)
    apart, after = scan_call(G, scan, d, dt, offsets, "sum", False, True, shift=1, out_shift=2)
    assert sc.same_bits(apart, results[0]) and sc.same_bits(after, d)


# ------------------------------------------------------------------------------------------------------------- wide indices


def test_out_of_place_stores_past_2_31_elements(G):
    """uint32, 2^31 + 2^20 elements in `data` and in `out` (8 GiB each): a workgroup-class segment that ends below element 2^31, a
    long one across it and a wave-class one behind it, out of place, inclusive Max.  Only the neighbourhood of the segments is
    filled (on the device) and compared: the values in the segments, the poison of `out` in the 4096 elements in front of and
    behind them and between them.  Skips where the memory is short."""
    import torch

    dt, op = 3, "max"
    wave, block, chunk, tile = class_limits(G, 4)
    boundary = 1 << 31
    total = boundary + (1 << 20)
    if torch.cuda.mem_get_info()[0] < 2 * 4 * total + (4 << 30):
        pytest.skip("needs 20 GiB of free HBM")
    lens = [block, 3, 0, 4 * chunk + 5, 2, wave]
    start = boundary - block - 3 - (2 * chunk + 1)
    offsets = start + np.concatenate([[0], np.cumsum(lens)])
    assert offsets[3] < boundary < offsets[4] and offsets[-1] < total
    assert [G.plan_scan_batch(n, 4)[0] for n in lens] == [2, 1, 0, 3, 1, 1]
    pad = 4096
    lo, hi = int(offsets[0]) - pad, int(offsets[-1]) + pad
    data = torch.empty(total, dtype=torch.int32, device="cuda")
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    data[lo:hi] = torch.randint(-(1 << 31), 1 << 31, (hi - lo,), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32)
    poison = int(poison_of(np.int32))
    out[lo:hi] = poison
    ot = device_offsets(offsets)
    scan = G.BlellochScan(dt)
    scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), len(lens), stream(), out_ptr=out.data_ptr(), op=op, inclusive=True)
    torch.cuda.synchronize()
    assert scan.read_batch() == {"wave": 3, "block": 1, "long": 1}
    d = data[lo:hi].cpu().numpy().view(np.uint32)
    got = out[lo:hi].cpu().numpy().view(np.uint32)
    want = sc.expected(d, dt, op, True, offsets - lo, base=np.full(hi - lo, poison, dtype=np.int32).view(np.uint32))
    bad = sc.first_difference(got, want, 1)
    assert bad is None, "element %d" % (lo + bad)
    del data, out
    torch.cuda.empty_cache()
