"""CPU tests of scan_ops_cases.py: the expected-value function against a plain Python loop, the identities, and the property the
GPU tests lean on -- the drawn inputs make every scan exact in the element type in ANY grouping of the operands."""
from fractions import Fraction

import numpy as np
import pytest

import scan_ops_cases as sc

KINDS = (False, True)


def small_offsets():
    lens = [0, 1, 2, 0, 0, 7, 33, 1, 0, 64]
    return np.concatenate([[3], 3 + np.cumsum(lens)]), 3 + sum(lens) + 4


@pytest.mark.parametrize("dt", range(12))
def test_expected_equals_a_plain_loop(dt):
    npdt, comps = sc.dtype_info(dt)
    offsets, total = small_offsets()
    for op in sc.OPS:
        rng = np.random.default_rng(1000 + 10 * dt + sc.OPS.index(op))
        d = sc.make_data(rng, dt, op, offsets, total)
        assert d.dtype == npdt and d.size == total * comps
        for inclusive in KINDS:
            want = sc.expected_by_loop(d, dt, op, inclusive, offsets)
            got = sc.expected(d, dt, op, inclusive, offsets)
            assert sc.same(op, npdt, got, want), (op, inclusive, sc.first_difference(got, want, comps))
            # outside the segments nothing changes; with a `base`, the base shows there
            assert sc.same_bits(got[:3 * comps], d[:3 * comps]) and sc.same_bits(got[int(offsets[-1]) * comps:], d[int(offsets[-1]) * comps:])
            base = np.full_like(d, 7)
            into = sc.expected(d, dt, op, inclusive, offsets, base=base)
            b, e = int(offsets[0]) * comps, int(offsets[-1]) * comps
            assert sc.same_bits(into[b:e], got[b:e]) and (into[:b] == 7).all() and (into[e:] == 7).all()


def test_identities_and_kinds_on_a_case_by_hand():
    d = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32)
    offsets = [1, 4, 4, 8]
    dt = 3  # uint
    assert sc.dtype_info(dt) == (np.uint32, 1)
    assert sc.expected(d, dt, "sum", False, offsets).tolist() == [3, 0, 1, 5, 0, 5, 14, 16]
    assert sc.expected(d, dt, "sum", True, offsets).tolist() == [3, 1, 5, 6, 5, 14, 16, 22]
    assert sc.expected(d, dt, "max", True, offsets).tolist() == [3, 1, 4, 4, 5, 9, 9, 9]
    assert sc.expected(d, dt, "max", False, offsets).tolist() == [3, 0, 1, 4, 0, 5, 9, 9]
    assert sc.expected(d, dt, "min", False, offsets).tolist() == [3, 0xFFFFFFFF, 1, 1, 0xFFFFFFFF, 5, 5, 2]
    assert sc.expected(d, dt, "mul", False, offsets).tolist() == [3, 1, 1, 4, 1, 5, 45, 90]
    f = np.array([2.0, -1.0, 0.5], dtype=np.float32)
    assert sc.expected(f, 0, "min", False, [0, 3]).tolist() == [np.inf, 2.0, -1.0]
    assert sc.expected(f, 0, "max", False, [0, 3]).tolist() == [-np.inf, 2.0, 2.0]
    i = np.array([-5, 7], dtype=np.int32)
    assert sc.expected(i, 2, "min", False, [0, 2]).tolist() == [2**31 - 1, -5]
    assert sc.expected(i, 2, "max", False, [0, 2]).tolist() == [-2**31, -5]
    assert sc.expected(np.array([0xFFFFFFFF, 3], dtype=np.uint32), 3, "mul", True, [0, 2]).tolist() == [0xFFFFFFFF, 0xFFFFFFFD]


def test_signed_zeros_compare_by_value_and_poison_by_bits():
    nan = np.array([0x7FC5A5A5], dtype=np.uint32).view(np.float32)[0]
    a = np.array([0.0, nan, 1.0], dtype=np.float32)
    b = np.array([-0.0, nan, 1.0], dtype=np.float32)
    assert sc.same_values(a, b) and not sc.same_bits(a, b)
    other_nan = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]
    assert not sc.same_values(a, np.array([0.0, other_nan, 1.0], dtype=np.float32))
    assert not sc.same_values(a, np.array([0.0, nan, 2.0], dtype=np.float32))


@pytest.mark.parametrize("dt", [0, 1, 5, 7])  # float, double, vec4, dvec4
def test_float_products_are_exact_in_any_grouping_and_of_any_subset(dt):
    """Every prefix of the exponents of a segment lies inside [-30, 30] (checked with fractions on the drawn data), so every
    contiguous sub-product is +-2^e with |e| <= 60.  And the exponents of a segment add up to at most 100 in absolute value, so
    the product of any subset of its elements -- a lane of the chunk kernel folds every 256th pack -- is a normal float32 too."""
    npdt, comps = sc.dtype_info(dt)
    lens = [0, 1, 5, 0, 700, 2049, 20000]
    offsets = np.concatenate([[2], 2 + np.cumsum(lens)])
    d = sc.make_data(np.random.default_rng(3), dt, "mul", offsets, int(offsets[-1]) + 3).reshape(-1, comps)
    lo, hi = Fraction(1, 2**sc.MUL_PREFIX_EXPONENT), Fraction(2**sc.MUL_PREFIX_EXPONENT)
    signs, reached = set(), 0
    for b, e in zip(offsets[:-1], offsets[1:]):
        for c in range(comps):
            acc = Fraction(1)
            for v in d[b:e, c].tolist():
                acc *= Fraction(v)
                assert lo <= abs(acc) <= hi
                assert abs(acc).numerator == 1 or abs(acc).denominator == 1  # a power of two
                signs.add(acc > 0)
                reached = max(reached, abs(acc), 1 / abs(acc))
            mantissa, exponent = np.frexp(np.abs(d[b:e, c].astype(np.float64)))
            assert (mantissa == 0.5).all() and np.abs(exponent - 1).sum() <= sc.MUL_TOTAL_EXPONENT
    assert signs == {True, False} and reached >= 8
    assert sc.MUL_TOTAL_EXPONENT < 126 and 2 * sc.MUL_PREFIX_EXPONENT < 126  # float32's normal range
    # a strided subset, as a lane of the chunk kernel folds it, in float32: exact
    x = d[int(offsets[-2]):int(offsets[-1]), 0]
    for lane in range(0, 64, 7):
        part = x[lane::256].astype(npdt)
        assert Fraction(float(np.multiply.reduce(part))) == np.prod([Fraction(float(v)) for v in part], dtype=object)


@pytest.mark.parametrize("dt", [0, 1, 4])
def test_float_sums_are_exact_in_any_grouping(dt):
    """length x max|k| < 2^24 eighths inside every segment: any partial sum of any subset is a multiple of 0.125 below 2^21."""
    npdt, comps = sc.dtype_info(dt)
    lens = [1, 100, 5000, 70000]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = sc.make_data(np.random.default_rng(4), dt, "sum", offsets, int(offsets[-1])).reshape(-1, comps)
    for b, e in zip(offsets[:-1], offsets[1:]):
        k = d[b:e].astype(np.float64) * 8
        assert (k == np.round(k)).all() and np.abs(k).sum(0).max() < 2**24


def test_integer_factors_are_odd_and_extremes_have_ties():
    offsets = [0, 5000]
    for dt in (2, 3, 9):
        d = sc.make_data(np.random.default_rng(5), dt, "mul", offsets, 5000)
        assert (d.view(np.uint32) & 1).all()
        want = sc.expected(d, dt, "mul", True, offsets)
        assert (want.view(np.uint32) & 1).all()  # no product collapses to 0
    for dt in (0, 2, 3):
        d = sc.make_data(np.random.default_rng(6), dt, "max", offsets, 5000)
        assert np.unique(d).size <= 32 and np.isfinite(d.astype(np.float64)).all()


def test_boundary_lengths_and_empty_segments():
    lens = sc.boundary_lengths(wave=512, block=16384, chunk=8192, tile=4096)
    assert lens == [0, 1, 2, 32, 33, 128, 129, 512, 513, 4095, 4096, 4097, 16384, 16385, 24577]
    spread = sc.with_empty_between([5, 6, 7])
    assert spread == [5, 0, 0, 6, 0, 0, 7]
