"""CPU tests of oracle/exact_inputs.py: the generators behind tests/test_gpu_scan_reduce_types.py keep their promises on every
shape that module runs, numpy's own sums pass the rounding bound before any kernel is asked to, and a double path that rounds
through float fails both kinds of check."""
import numpy as np
import pytest

import exact_inputs as X
from oracle import dtype_info

INT_KINDS = tuple(dt for dt in X.ALL_TYPES if not X.is_float_kind(dt))


def test_significant_bits():
    m = np.array([0, 1, -1, 6, 2**24, 2**24 + 1, -(2**40 - 1), 2**52 + 2**20], dtype=np.int64)
    assert X.significant_bits(m).tolist() == [0, 1, 1, 2, 1, 25, 40, 33]


def test_chunk_sizes_follow_the_element_size():
    assert [X.scan_chunk(dt) for dt in (0, 1, 4, 5, 6, 7)] == [4096, 2048, 2048, 1024, 1024, 1024]
    assert X.two_level_count(3) == 2**24 + 1 and X.two_level_count(8) == 2**22 + 1 and X.two_level_count(11) == 2**20 + 1


def test_shapes_take_the_kernels_they_are_meant_for():
    """The host's choice between the small-partitions kernel and the chunked ones, restated from ScanCfg: a wave spans 1024,
    512 or 256 elements, so 2048 x 37 is chunked for every type and 256 x 67 is not for any."""
    assert [X.scan_wave_elems(dt) for dt in (0, 1, 4, 5, 6, 7)] == [1024, 512, 512, 256, 256, 256]
    for dt in X.ALL_TYPES:
        assert not any(X.takes_small_partitions_kernel(dt, c, p) for c, p in X.SCAN_POW2_SHAPES)
        assert all(X.takes_small_partitions_kernel(dt, c, p) for c, p in X.small_partition_shapes(dt))
        assert (256, 67) in X.small_partition_shapes(dt)
        assert ((512, 37) in X.small_partition_shapes(dt)) == (X.elem_bytes(dt) <= 8)


def test_the_references_own_error_fits_between_gamma_k_minus_1_and_gamma_k():
    """The tolerance gamma_k * sum|x| is the theorem's gamma_{k-1} * sum|x| plus about u * sum|x|; the reference's own error,
    at most gamma_a(u_ref) * sum|x| for its a additions per value, must fit into that step with room for sum|x| itself."""
    for dt in X.FLOAT_KINDS:
        u, u_ref = X.unit_roundoff(dt), float(np.finfo(X.reference_float(dt)).eps) / 2
        for k, scan in [(c, True) for c, _ in _rounding_shapes(dt)] + [(n, False) for n in X.REDUCE_ROUNDING_SIZES]:
            assert float(X.gamma(X.reference_additions(k, scan), u_ref)) <= u / 8, (dt, k)
    assert X.reference_additions(8193, True) == 193 and X.reference_additions(3000001, False) == 22
    ints = np.arange(1, 1001, dtype=np.float64).reshape(500, 2)
    assert X._tree_sum(ints).tolist() == [250000.0, 250500.0]
    x = np.random.default_rng(1).standard_normal((2, 1000, 3)).astype(np.longdouble)
    assert np.allclose(X._blocked_cumsum(x).astype(np.float64), np.cumsum(x.astype(np.float64), axis=1), rtol=0, atol=1e-9)
    exact = np.arange(1, 301, dtype=np.float64).reshape(1, 300, 1)
    assert (X._blocked_cumsum(exact) == np.cumsum(exact, axis=1)).all()


@pytest.mark.parametrize("dt", X.FLOAT_KINDS)
def test_exact_sums_hold_their_budget_on_every_shape(dt):
    """sum(|m|) < 2^p per component, the values are m * 2^-s exactly, and the double kinds need more than 24 bits; then the
    component type's own arithmetic gives the expected bits forwards, backwards and pairwise."""
    npdt, comps = dtype_info(dt)
    p = X.mantissa_bits(dt)
    for n, neg in X.exact_sum_shapes(dt):
        top = X.exact_sum_top(dt, n)
        # the budget by arithmetic, for every shape: n values of at most `top`, or a quarter of n ones (six sigma above the mean)
        assert (n * top if top else n / 4 + 6 * (n * 3 / 16) ** 0.5) < 2**p
        if dt in X.DOUBLE_KINDS:
            # uniform |m| <= top >= 2^28: at most 1/4 of them are shorter than 27 bits, and 1/8 of the rest end in 3 zero bits or
            # more, so at least 0.75 * 0.875 of the values need more than 24 bits
            assert top >= 2**28
        if n * comps > 2**21:
            continue  # (the arithmetic above is the check; exact_sums asserts its budget on every value whenever it runs)
        c = X.exact_sums(dt, n, X.seed_of(dt, n), neg)
        assert c.data.dtype == npdt and c.data.size == n * comps
        assert int(np.abs(c.m).sum(axis=0).max()) < 2**c.p
        assert (c.data.reshape(n, comps).astype(np.float64) * 2.0**c.s == c.m).all()
        if dt in X.DOUBLE_KINDS:
            bits = X.significant_bits(c.m)
            assert (bits > 24).mean() > 0.5
            assert np.median(bits) >= min(40, 52 - int(np.ceil(np.log2(n))) - 3)  # about 30 bits at 2^22, 40 at 2^12
        if neg == 0:
            assert int(c.m.sum(axis=0).max()) >= 2**(c.p - 2)  # the prefixes climb into the top bits
        x = c.data.reshape(n, comps)
        want = X.expected_sum(c)
        assert want.dtype == npdt
        for got in (x.sum(axis=0, dtype=npdt), x[::-1].sum(axis=0, dtype=npdt), np.add.reduce(np.ascontiguousarray(x.T), axis=1, dtype=npdt)):
            assert (got == want).all(), (dt, n)
    count, parts = X.SCAN_POW2_SHAPES[0]
    c = X.exact_sums(dt, count * parts, X.seed_of(dt, count * parts))
    x = c.data.reshape(parts, count, comps)
    seq = np.cumsum(x, axis=1, dtype=npdt) - x  # exact data: the subtraction is exact too
    assert (X.expected_scan(c, count, parts) == seq.reshape(-1)).all()


@pytest.mark.parametrize("dt", INT_KINDS)
def test_integer_sums_and_products_wrap_like_python_integers(dt):
    npdt, comps = dtype_info(dt)
    n = 1027
    c = X.exact_sums(dt, n, X.seed_of(dt, n))
    u = c.data.view(np.uint32).reshape(n, comps)
    assert u.max() > 2**31 and u.min() < 2**31  # the full range
    for k in range(comps):
        col = [int(v) for v in u[:, k]]
        assert int(X.expected_sum(c).view(np.uint32)[k]) == sum(col) % 2**32
        scan = X.expected_scan(c, n, 1).view(np.uint32).reshape(n, comps)[:, k]
        assert [int(v) for v in scan[:5]] == [sum(col[:i]) % 2**32 for i in range(5)] and int(scan[-1]) == sum(col[:-1]) % 2**32
    for n in X.REDUCE_NEUTRAL_SIZES:
        c = X.exact_products(dt, n, X.seed_of(dt, n, X.OP_MUL))
        u = c.data.view(np.uint32).reshape(n, comps)
        assert (u & 1).all()  # odd factors: the product never collapses to 0
        if n <= 1027:
            for k in range(comps):
                prod = 1
                for v in u[:, k]:
                    prod = prod * int(v) % 2**32
                assert int(c.expected.view(np.uint32)[k]) == prod
                assert n == 1 or prod != int(u[0, k])  # the product does wrap
        assert not (c.expected.view(np.uint32) == 1).any() and (c.expected.view(np.uint32) & 1).all()


@pytest.mark.parametrize("dt", X.FLOAT_KINDS)
def test_float_products_stay_powers_of_two_in_the_normal_range(dt):
    npdt, comps = dtype_info(dt)
    for n in sorted(set(X.REDUCE_NEUTRAL_SIZES + X.REDUCE_OFFSET_SIZES)):
        if n * comps > 2**22:
            continue  # (the components are drawn alike: the scalar types cover the largest size)
        c = X.exact_products(dt, n, X.seed_of(dt, n, X.OP_MUL))
        x = c.data.reshape(n, comps)
        assert np.isin(np.abs(x), [0.5, 1.0, 2.0]).all()
        assert (c.data != 1).sum() <= X.MAX_NON_ONE
        assert (c.data != 1).sum() == min(n * comps, X.MAX_NON_ONE)  # short arrays: no factor of 1 at all
        assert np.abs(np.log2(np.abs(x))).sum() <= X.MAX_NON_ONE  # exponent budget: every subset product within 2^+-100
        assert 100 < -np.finfo(npdt).minexp
        for got in (np.multiply.reduce(x, axis=0, dtype=npdt), np.multiply.reduce(x[::-1], axis=0, dtype=npdt)):
            assert (got == c.expected).all()


@pytest.mark.parametrize("dt", X.ALL_TYPES)
@pytest.mark.parametrize("op", [X.OP_MIN, X.OP_MAX])
def test_extremes_sit_where_asked_and_zero_is_not_neutral(dt, op):
    npdt, comps = dtype_info(dt)
    vec = max(1, 16 // X.elem_bytes(dt))
    for n in (1, 3, 5, 255, 1027, 262147):
        for place in X.EXTREME_PLACES:
            at = X.extreme_index(dt, n, place)
            assert at == {"first": 0, "last": n - 1}.get(place, at) and 0 <= at < n
            if place == "tail" and n % vec:
                assert n - n % vec <= at < n  # inside what whole vectors leave over
            for variant in X.extreme_variants(dt):
                c = X.extreme_case(dt, n, op, place, X.seed_of(dt, n, op), variant)
                x = c.data.reshape(n, comps)
                assert not (X.is_float_kind(dt) and np.isnan(x).any())
                want = x.min(axis=0) if op == X.OP_MIN else x.max(axis=0)
                assert (want == c.expected).all() and c.index == at
                if variant == "plain":
                    assert (x[at] == c.expected).all() and (x != 0).all()
                    assert ((np.delete(x, at, axis=0) == c.expected).sum() == 0)  # the extreme is in one place only
                    if op == X.OP_MIN or npdt == np.uint32:
                        assert (c.expected > 0).all()  # a leaked 0 would win a min
                    else:
                        assert (c.expected < 0).all()  # a leaked 0 would win a max
                if variant == "winning_inf":
                    assert np.isinf(c.expected).all() and (np.sign(c.expected) == (1 if op == X.OP_MAX else -1)).all()
                if variant == "losing_inf" and n > 1:
                    assert np.isinf(x).any() and np.isfinite(c.expected).all()
                if variant == "zeros" and n > 2:
                    assert (c.expected == 0).all() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()


def _rounding_shapes(dt):
    shapes = [X.ROUNDING_SCAN_SHAPE] + ([s for s in X.CHAINED_SHAPES] if dt == 0 else [])
    return shapes


@pytest.mark.parametrize("dt", X.FLOAT_KINDS)
def test_numpys_own_sums_meet_the_rounding_bound(dt):
    """The component type's sequential cumsum and pairwise sum are correct summations, so they must sit inside the bound that
    the kernels are held to; and not trivially: the data do round."""
    npdt, comps = dtype_info(dt)
    for count, parts in _rounding_shapes(dt):
        d = X.rounding_data(dt, count * parts, X.seed_of(dt, count * parts, 5))
        ref, bound = X.rounding_scan_reference(dt, d, count, parts)
        x = d.reshape(parts, count, comps)
        got = np.concatenate([np.zeros((parts, 1, comps), npdt), np.cumsum(x, axis=1, dtype=npdt)[:, :-1]], axis=1)
        assert X.within_bound(got.reshape(-1), ref, bound).all()
        assert (bound.reshape(parts, count, comps)[:, 0] == 0).all() and (bound.reshape(parts, count, comps)[:, 1:] > 0).all()
        assert (got.reshape(-1).astype(ref.dtype) != ref).mean() > 0.5  # these sums round
    for n in X.REDUCE_ROUNDING_SIZES:
        if n * comps > 2**22:
            continue  # (the components are drawn alike: the scalar types cover the largest size)
        d = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
        ref, bound = X.rounding_sum_reference(dt, d)
        x = np.ascontiguousarray(d.reshape(n, comps).T)
        for got in (np.add.reduce(x, axis=1, dtype=npdt), np.cumsum(x, axis=1, dtype=npdt)[:, -1]):  # pairwise, sequential
            assert X.within_bound(got, ref, bound).all()


@pytest.mark.parametrize("dt", X.DOUBLE_KINDS)
def test_a_double_path_through_float_fails_both_checks(dt):
    """What the GPU tests are for: a reduction or scan of a double kind that accumulates in float, or that stores its partial
    sums as float between two stages, returns other bits on the exact inputs; the float accumulation also leaves the bound on
    the rounding inputs (a few thousand parked partials do not: at 3 * 10^6 elements the bound is only 2^29 / k = 180 times
    tighter than float, which is why the exact inputs come first)."""
    npdt, comps = dtype_info(dt)
    f32 = np.float32
    for n in X.REDUCE_DOUBLE_SIZES:
        if n * comps > 2**22:
            continue  # (the components are drawn alike: the scalar types cover the largest size)
        c = X.exact_sums(dt, n, X.seed_of(dt, n))
        x = c.data.reshape(n, comps)
        want = X.expected_sum(c)
        assert (x.sum(axis=0) == want).all()  # the honest double sum passes
        through_float = x.astype(f32).sum(axis=0, dtype=f32).astype(npdt)
        assert (through_float != want).all(), n
        if 1024 < n < 2**20:  # two stages: double arithmetic, partials of 1024 elements parked in float
            pad = np.concatenate([x, np.zeros((-n % 1024, comps), npdt)]).reshape(-1, 1024, comps)
            parked = pad.sum(axis=1).astype(f32).astype(npdt).sum(axis=0)
            assert (parked != want).all(), n
    for n in X.REDUCE_ROUNDING_SIZES:
        if n * comps > 2**22:
            continue  # (the components are drawn alike: the scalar types cover the largest size)
        d = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
        ref, bound = X.rounding_sum_reference(dt, d)
        x = d.reshape(n, comps)
        assert X.within_bound(x.sum(axis=0), ref, bound).all()
        assert not X.within_bound(x.astype(f32).sum(axis=0, dtype=f32).astype(npdt), ref, bound).any()
    for count, parts in (X.SCAN_POW2_SHAPES[0], X.ROUNDING_SCAN_SHAPE):
        n = count * parts
        c = X.exact_sums(dt, n, X.seed_of(dt, n))
        x = c.data.reshape(parts, count, comps)
        sim = np.cumsum(x.astype(f32), axis=1, dtype=f32).astype(npdt)[:, :-1]
        want = X.expected_scan(c, count, parts).reshape(parts, count, comps)[:, 1:]
        assert (sim != want).mean() > 0.9
        d = X.rounding_data(dt, n, X.seed_of(dt, n, 5))
        ref, bound = X.rounding_scan_reference(dt, d, count, parts)
        x = d.reshape(parts, count, comps)
        sim = np.concatenate([np.zeros((parts, 1, comps), npdt), np.cumsum(x.astype(f32), axis=1, dtype=f32).astype(npdt)[:, :-1]], axis=1)
        assert X.within_bound(sim.reshape(-1), ref, bound).mean() < 0.1
