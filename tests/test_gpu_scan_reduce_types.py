"""GPU tests of glu::BlellochScan and glu::Reduce on inputs whose expected result does not depend on the order of the operations
(oracle/exact_inputs.py; tests/test_exact_inputs.py checks those generators on the CPU): the 8-byte component types at their full
53 bits, the deeper scan levels and the unaligned kernels of every element width, reductions where neither 0 nor 1 is neutral,
integer products that wrap, and float sums that round, held to the bound that every correct summation meets.

Every reduce here also checks that nothing but element 0 was written, and every scan or reduce that starts inside an allocation
that the bytes in front of it are untouched."""
import numpy as np
import pytest

import exact_inputs as X
from oracle import dtype_info

pytestmark = pytest.mark.gpu

GUARD = 0xA5  # byte in front of and behind the arrays that start or end inside an allocation
WIDE_TYPES = tuple(dt for dt in X.ALL_TYPES if X.elem_bytes(dt) >= 8)
NARROW_TYPES = tuple(dt for dt in X.ALL_TYPES if X.elem_bytes(dt) <= 8)  # the seven 4- and 8-byte types
OPS = (X.OP_SUM, X.OP_MUL, X.OP_MIN, X.OP_MAX)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


# ---- helpers ---------------------------------------------------------------------------------------------------------
def run_scan(G, scan, dt, data, count, parts, lead=0, buffer_call=False):
    """Scans `data` (flat, count * parts elements) in place on the device, `lead` elements into its allocation; returns the
    result, flat.  buffer_call: through BlellochScan::operator() (power-of-two counts) instead of the raw-pointer entry."""
    npdt = dtype_info(dt)[0]
    front = lead * X.elem_bytes(dt)
    host = np.concatenate([np.full(front, GUARD, np.uint8), data.view(np.uint8)])
    b = G.ShaderStorageBuffer(host)
    if buffer_call:
        assert lead == 0
        scan(b, count, parts)
    else:
        scan.run_ptr(b.device_ptr() + front, count, parts)
    got = b.get_data(np.uint8)
    assert (got[:front] == GUARD).all(), "the scan wrote in front of its array"
    return got[front:].view(npdt)


def assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first differences at", bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist(), "of", bad.size)


def scan_exact(G, scan, dt, count, parts, lead=0, neg=0.5, buffer_call=False):
    n = count * parts
    case = X.exact_sums(dt, n, X.seed_of(dt, n), neg)
    got = run_scan(G, scan, dt, case.data, count, parts, lead, buffer_call)
    assert_same(got, X.expected_scan(case, count, parts), (dt, count, parts, lead))


def scan_rounding(G, scan, dt, count, parts):
    n = count * parts
    data = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
    ref, bound = X.rounding_scan_reference(dt, data, count, parts)
    got = run_scan(G, scan, dt, data, count, parts)
    err = np.abs(got.astype(ref.dtype) - ref)
    print("scan dt %d count %d x %d: largest error / bound = %.3g" % (dt, count, parts, float((err[bound > 0] / bound[bound > 0]).max())))
    bad = np.flatnonzero(~X.within_bound(got, ref, bound))
    assert bad.size == 0, (dt, count, parts, bad[:4].tolist(), err[bad[:4]].tolist(), bound[bad[:4]].tolist())


def run_reduce(G, red, dt, data, n, lead=0, pad=0):
    """Reduces `data` (flat, n elements) on the device, `lead` elements into its allocation and with `pad` bytes behind it;
    returns element 0 afterwards, having checked that no other byte of the allocation changed."""
    npdt = dtype_info(dt)[0]
    es = X.elem_bytes(dt)
    front = lead * es
    host = np.concatenate([np.full(front, GUARD, np.uint8), data.view(np.uint8), np.full(pad, GUARD, np.uint8)])
    assert host.size == front + n * es + pad
    b = G.ShaderStorageBuffer(host)
    red.run_ptr(b.device_ptr() + front, n)
    got = b.get_data(np.uint8)
    assert (got[:front] == host[:front]).all(), "the reduce wrote in front of its array"
    assert (got[front + es:] == host[front + es:]).all(), "the reduce wrote behind element 0"
    return got[front:front + es].view(npdt)


def reduce_cases(dt, op, n, every_place):
    """(label, data, expected) of generators 1 - 4 for the operator.  Min and max: every place of the extreme and every float
    variant (every_place), or the extreme in the vector tail with every variant plus the plain data at the other two places."""
    if op == X.OP_SUM:
        case = X.exact_sums(dt, n, X.seed_of(dt, n))
        yield "sum", case.data, X.expected_sum(case)
    elif op == X.OP_MUL:
        case = X.exact_products(dt, n, X.seed_of(dt, n, op))
        yield "product", case.data, case.expected
    else:
        for place in X.EXTREME_PLACES:
            for variant in X.extreme_variants(dt):
                if every_place or place == "tail" or variant == "plain":
                    case = X.extreme_case(dt, n, op, place, X.seed_of(dt, n, op), variant)
                    yield (place, variant), case.data, case.expected


def reduce_all_cases(G, red, dt, op, n, lead=0, pad=0, every_place=True):
    for label, data, want in reduce_cases(dt, op, n, every_place):
        got = run_reduce(G, red, dt, data, n, lead, pad)
        assert (got == want).all(), (dt, op, n, label, got.tolist(), want.tolist())  # (== is by value: either zero passes)


# ---- scan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", X.ALL_TYPES)
def test_scan_keeps_every_bit_at_power_of_two_counts(G, dt):
    """8192 x 3 and 2048 x 37 through BlellochScan::operator(): the chunked kernels with several chunks per partition and
    with one or two (no type's wave spans 2048 elements, so neither shape takes the small-partitions kernel: the next test
    does).  The double kinds carry about 40 significant bits here."""
    scan = G.BlellochScan(dt)
    for count, parts in X.SCAN_POW2_SHAPES:
        assert not X.takes_small_partitions_kernel(dt, count, parts)
        scan_exact(G, scan, dt, count, parts, buffer_call=True)


@pytest.mark.parametrize("dt", X.ALL_TYPES)
def test_scan_of_small_partitions_keeps_every_bit(G, dt):
    """scan_small_partitions_kernel (partitions of at most one wave's span packed into a workgroup: its own segmented wave
    scan and running sum) on data that need every mantissa bit: 256 x 67 for every width, 512 x 37 where a partition then
    spans several groups of a wave (the 4- and 8-byte types), from the head of the allocation and, for those types, one
    element into it (4 or 8 modulo 16: the kernel's element-by-element loads and stores)."""
    scan = G.BlellochScan(dt)
    for count, parts in X.small_partition_shapes(dt):
        assert X.takes_small_partitions_kernel(dt, count, parts)
        scan_exact(G, scan, dt, count, parts, buffer_call=True)
        if X.elem_bytes(dt) <= 8:
            scan_exact(G, scan, dt, count, parts, lead=1)


@pytest.mark.parametrize("dt", X.ALL_TYPES)
def test_scan_with_two_levels_of_chunk_sums(G, monkeypatch, dt):
    """CHUNK^2 + 1 elements: the chunk sums span more than one chunk themselves, so the sums of sums are scanned and carried
    back, for every element width (CHUNK as ScanCfg derives it from the element size: exact_inputs.scan_chunk).  The 4-byte
    types are kept off the single-pass scan; the 8-byte types also run two partitions, the second of which starts at an
    address of 8 modulo 16 because the count is odd."""
    if X.elem_bytes(dt) == 4:
        monkeypatch.setenv("GLU_HIP_SCAN_CHAINED", "0")
    chunk = X.scan_chunk(dt)
    count = X.two_level_count(dt)
    sums = -(-count // chunk)  # chunk sums per partition
    assert sums > chunk and -(-sums // chunk) == 2  # they span two chunks: a second level of sums
    scan = G.BlellochScan(dt)
    for parts in X.two_level_partitions(dt):
        scan_exact(G, scan, dt, count, parts)


@pytest.mark.parametrize("dt", WIDE_TYPES)
def test_scan_wide_types_unaligned_and_not_a_power_of_two(G, dt):
    """3, 2049 and 4097 elements x 3 partitions: one chunk and several, counts that leave a partial vector and a partial chunk.
    The 8-byte types take the unaligned kernels (an odd count puts the second partition at 8 modulo 16) and are also started
    one element into the allocation; the 16- and 32-byte types must be 16-byte aligned, so for them the counts are the case."""
    scan = G.BlellochScan(dt)
    for count in X.SCAN_WIDE_COUNTS:
        for lead in ((0, 1) if X.elem_bytes(dt) == 8 else (0,)):
            scan_exact(G, scan, dt, count, 3, lead=lead)


def test_chained_scan_of_floats_that_need_all_24_bits(G, monkeypatch):
    """The single-pass scan from two chunks up, unaligned (32768 * 3 + 5 elements x 2) and aligned over 64 chunks: exact inputs
    of mixed sign, exact inputs that are all positive so that the prefixes climb to 2^23 and beyond, and rounding inputs
    against the bound (the look-back changes the order of the additions, not their number)."""
    monkeypatch.setenv("GLU_HIP_SCAN_CHAINED", "2")
    scan = G.BlellochScan(G.DataType_Float)
    for count, parts in X.CHAINED_SHAPES:
        for neg in (0.5, 0.0):
            scan_exact(G, scan, G.DataType_Float, count, parts, neg=neg)
        scan_rounding(G, scan, G.DataType_Float, count, parts)


@pytest.mark.parametrize("dt", X.FLOAT_KINDS)
def test_scan_of_rounding_floats_stays_inside_the_bound(G, dt):
    """8193 x 3 elements, where additions round: element i is within gamma_i * sum(|x_j|, j < i) of the reference, per component.
    For the double kinds that is about 2^29 / i tighter than float arithmetic could meet."""
    scan_rounding(G, G.BlellochScan(dt), dt, *X.ROUNDING_SCAN_SHAPE)


# ---- reduce ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", NARROW_TYPES)
def test_reduce_from_an_address_that_is_not_a_multiple_of_16(G, dt, op):
    """One element into the allocation: the kernels that load element by element, and the host's block count for them, with one
    workgroup (1, 5, 1000) and two stages (262147, 3000001)."""
    red = G.Reduce(dt, op)
    for n in X.REDUCE_OFFSET_SIZES:
        reduce_all_cases(G, red, dt, op, n, lead=1, every_place=n <= 1000)


@pytest.mark.parametrize("dt", X.DOUBLE_KINDS)
def test_reduce_sums_doubles_at_full_precision(G, dt):
    """Values of 30 (3000001 elements) to 50 (7 elements) significant bits whose sum is exact in any order."""
    red = G.Reduce(dt, X.OP_SUM)
    for n in X.REDUCE_DOUBLE_SIZES:
        reduce_all_cases(G, red, dt, X.OP_SUM, n)


@pytest.mark.parametrize("op", (X.OP_MUL, X.OP_MIN, X.OP_MAX))
@pytest.mark.parametrize("dt", X.ALL_TYPES)
def test_reduce_where_zero_and_one_are_not_neutral(G, dt, op):
    """Max over negative, min over positive data, the extreme at the first and the last element and in the tail behind the whole
    vectors, +-inf and both zeros for the float kinds; products of odd integers that wrap and of +-2^k without a factor of 1
    where the array is short: a start value or a lane without elements that leaks into the result changes it."""
    red = G.Reduce(dt, op)
    for n in X.REDUCE_NEUTRAL_SIZES:
        reduce_all_cases(G, red, dt, op, n)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", X.ALL_TYPES)
def test_reduce_in_two_stages_writes_one_element(G, dt, op):
    """300000 elements take the two-stage path: the first stage must write to the partials only, the second to element 0 only.
    Every other byte, 64 bytes behind the last element included, equals the input (run_reduce checks it)."""
    reduce_all_cases(G, G.Reduce(dt, op), dt, op, X.REDUCE_TWO_STAGE_SIZE, pad=64, every_place=False)


@pytest.mark.parametrize("dt", X.FLOAT_KINDS)
def test_reduce_of_rounding_floats_stays_inside_the_bound(G, dt):
    """|result - reference| <= gamma_n * sum(|x_i|) per component, the reference in float64 (long double for the double kinds)."""
    red = G.Reduce(dt, X.OP_SUM)
    for n in X.REDUCE_ROUNDING_SIZES:
        data = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
        ref, bound = X.rounding_sum_reference(dt, data)
        got = run_reduce(G, red, dt, data, n)
        err = np.abs(got.astype(ref.dtype) - ref)
        print("reduce dt %d n %d: largest error / bound = %.3g" % (dt, n, float((err / bound).max())))
        assert X.within_bound(got, ref, bound).all(), (dt, n, err.tolist(), bound.tolist())
