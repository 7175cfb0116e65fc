"""Inputs for glu::BlellochScan and glu::Reduce whose expected result does not depend on the order of the operations, and
rounding inputs with the tolerance that any correct summation meets.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.  Nothing here needs a GPU.

A kernel is free to add, multiply or compare in any tree it likes, so a test that wants `==` needs data on which every tree
gives the same bits.  The generators below build such data for each of the 12 element types (oracle.dtype_info) and compute
the expected values in integers:

  1. exact_sums (float kinds): x = m * 2^-s with integer m and sum(|m|) < 2^p over the whole array, per component (p = 24
     for float, 53 for double).  Every partial sum over every subset is an integer below 2^p times 2^-s: representable, so no
     addition ever rounds.  For the double kinds |m| goes up to 2^53 / n / 2, so most values need more than 24 significant
     bits and a path that drops to float anywhere cannot return the same bits (asserted here).
  2. exact_sums (integer kinds) and exact_products (integer kinds): the full 32-bit range, odd factors for the products (a
     product of odd numbers never collapses to 0); expected values modulo 2^32 from 64-bit arithmetic.
  3. exact_products (float kinds): +-2^k, k in {-1, 0, 1}, at most 100 entries different from 1, so every subset product is a
     power of two between 2^-100 and 2^100: normal in float and double, exact in any order.
  4. extreme_case: min / max data on which 0 is NOT neutral (max over all-negative, min over all-positive data; unsigned data
     are positive for both), with the extreme where the caller asks: first element, last element, or inside the tail that a
     16-byte vector loop leaves over.  Float kinds also get +-inf and the pair -0.0 / +0.0 (compare by value: either zero is
     a correct answer).
  5. rounding_data: normal values times log-uniform magnitudes, mixed sign, where additions do round.  A sum of k numbers
     in any order in precision u is within gamma_k * sum(|x_i|) of the exact sum, gamma_k = k*u / (1 - k*u) (Higham, Accuracy
     and Stability of Numerical Algorithms, section 4.2); u = 2^-24 for float, 2^-53 for double.  That is the tolerance, per
     component and per element (for the exclusive scan k is the element's index), with no margin: it is a theorem, not a
     measurement.  Added zeros are exact and do not count; a different order of the additions does not change their number.
     The reference is float64 for the float kinds and np.longdouble (64-bit mantissa) for the double kinds.  The theorem has
     k - 1 additions; the step from gamma_{k-1} to gamma_k, about u * sum(|x|), is the room for the reference's own error,
     so that error has to stay below it: the reference scans in blocks of 128 (_blocked_cumsum: at most 127 + k / 128 + 1
     additions per value) and sums as a balanced tree (_tree_sum: log2 k additions) in a precision 2^11 (double kinds) or
     2^29 (float kinds) times finer: below u / 8 * sum(|x|) for every k used here, the same again for sum(|x|) itself.

No generator emits a NaN.  The operators are `a < b ? a : b` and `a > b ? a : b`: with a NaN the answer depends on the order
of the comparisons, and the reference implementation promises nothing there either, so there is nothing to assert.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import dtype_info

OP_SUM, OP_MUL, OP_MIN, OP_MAX = 0, 1, 2, 3
FLOAT_KINDS = (0, 1, 4, 5, 6, 7)      # float, double, vec2, vec4, dvec2, dvec4
DOUBLE_KINDS = (1, 6, 7)
ALL_TYPES = tuple(range(12))
MAX_NON_ONE = 100                     # generator 3: entries different from 1


def is_float_kind(dt):
    return np.issubdtype(dtype_info(dt)[0], np.floating)


def elem_bytes(dt):
    npdt, comps = dtype_info(dt)
    return np.dtype(npdt).itemsize * comps


def mantissa_bits(dt):
    """p: integers below 2^p are exact in the component type (32 for the integer kinds: arithmetic modulo 2^32)."""
    npdt = dtype_info(dt)[0]
    return {np.float32: 24, np.float64: 53}.get(npdt, 32)


def unit_roundoff(dt):
    return 2.0 ** -mantissa_bits(dt)


def significant_bits(m):
    """Bits between the highest and the lowest set bit of |m|, inclusive (0 for 0): what a mantissa has to hold."""
    a = np.abs(np.asarray(m, dtype=np.int64)).astype(np.uint64)
    assert not a.size or int(a.max()) < 2**53
    out = np.zeros(a.shape, dtype=np.int64)
    nz = a != 0
    v = a[nz]
    low = v & (~v + np.uint64(1))                       # lowest set bit
    v = v // low                                        # odd now
    out[nz] = np.frexp(v.astype(np.float64))[1]         # bit length (|m| < 2^53 is exact in float64)
    return out


# ---- 1 and 2: sums -------------------------------------------------------------------------------------------------
def exact_sum_top(dt, n):
    """Largest |m| that exact_sums draws for n elements of a float kind (0: more elements than 2^p, the data are zeros and a
    quarter of +-1)."""
    if mantissa_bits(dt) == 53:
        return 2**53 // n // 2                          # sum(|m|) <= n * top <= 2^52
    return (2**24 - 1) // n                             # sum(|m|) <= n * top < 2^24


def exact_sums(dt, n, seed, neg=0.5):
    """n elements of type dt whose sums are exact in any order.  Returns a namespace: data (flat, n * comps values), m (int64,
    n x comps), s (x = m * 2^-s; None for the integer kinds), p.  `neg` is the share of negative values among the signed kinds:
    0 gives prefix sums that climb through all p bits."""
    npdt, comps = dtype_info(dt)
    rng = np.random.default_rng(seed)
    p = mantissa_bits(dt)
    if not is_float_kind(dt):
        u = rng.integers(0, 2**32, (n, comps), dtype=np.uint32)
        return SimpleNamespace(dt=dt, n=n, data=u.view(npdt).reshape(-1), m=u.astype(np.int64), s=None, p=32)
    s = 5 if p == 24 else 17
    top = exact_sum_top(dt, n)
    if top >= 1:
        mag = rng.integers(0, top + 1, (n, comps), dtype=np.int64)
    else:                                               # more elements than 2^p: zeros and a quarter of ones
        mag = (rng.integers(0, 4, (n, comps), dtype=np.int8) == 0).astype(np.int64)
    m = np.where(rng.random((n, comps), dtype=np.float32) < neg, -mag, mag)
    assert int(np.abs(m).sum(axis=0).max()) < 2**p, "sum(|m|) must stay below 2^p"
    if p == 53:
        assert (significant_bits(m) > 24).mean() > 0.5, "most double values must need more than float's 24 bits"
    data = (m.astype(np.float64) * 2.0 ** -s).astype(npdt)  # |m| < 2^53: exact in float64, then exact in npdt
    return SimpleNamespace(dt=dt, n=n, data=data.reshape(-1), m=m, s=s, p=p)


def _from_integers(case, v):
    """Integer results (int64, any shape) as values of the case's component type."""
    npdt = dtype_info(case.dt)[0]
    if case.s is None:
        return (v & 0xFFFFFFFF).astype(np.uint32).view(npdt)
    return (v.astype(np.float64) * 2.0 ** -case.s).astype(npdt)


def expected_sum(case):
    """The sum of all n elements, per component."""
    return _from_integers(case, case.m.sum(axis=0, dtype=np.int64))


def expected_scan(case, count, parts):
    """The in-place exclusive scan of `parts` adjacent partitions of `count` elements, flat like case.data.  int64 holds every
    prefix: below 2^53 for the float kinds, below 2^32 * n for the integer kinds (taken modulo 2^32)."""
    comps = case.m.shape[1]
    assert count * parts == case.n and case.n < 2**31
    m = case.m.reshape(parts, count, comps)
    ex = np.cumsum(m, axis=1, dtype=np.int64) - m
    return _from_integers(case, ex).reshape(-1)


# ---- 2 and 3: products ---------------------------------------------------------------------------------------------
def _product_mod_2_32(u):
    """Product of the rows of u (uint64 values below 2^32, n x comps) modulo 2^32, as a tree: the product is associative."""
    while u.shape[0] > 1:
        if u.shape[0] & 1:
            u = np.concatenate([u, np.ones((1, u.shape[1]), dtype=np.uint64)])
        u = (u[0::2] * u[1::2]) & np.uint64(0xFFFFFFFF)
    return u[0]


def exact_products(dt, n, seed):
    """n elements whose product is exact in any order.  Returns a namespace: data (flat), expected (comps values).
    Integer kinds: odd 32-bit factors, expected modulo 2^32.  Float kinds: +-2^k with k in {-1, 0, 1}, at most MAX_NON_ONE
    entries of the whole array different from 1 (all of them where the array is that short), expected from the exponents' sum."""
    npdt, comps = dtype_info(dt)
    rng = np.random.default_rng(seed)
    if not is_float_kind(dt):
        u = rng.integers(0, 2**32, (n, comps), dtype=np.uint32) | np.uint32(1)
        exp = _product_mod_2_32(u.astype(np.uint64)).astype(np.uint32).view(npdt)
        return SimpleNamespace(dt=dt, n=n, data=u.view(npdt).reshape(-1), expected=exp)
    total = n * comps
    k = np.zeros(total, dtype=np.int64)
    negative = np.zeros(total, dtype=bool)
    where = rng.choice(total, min(MAX_NON_ONE, total), replace=False)
    k[where] = rng.choice([-1, 1], where.size)              # never 2^0 = 1 ...
    negative[where] = rng.random(where.size) < 0.5
    flip = where[: where.size // 4]                         # ... except as -1
    k[flip], negative[flip] = 0, True
    data = np.where(negative, -1.0, 1.0) * 2.0 ** k.astype(np.float64)
    assert (data != 1).sum() <= MAX_NON_ONE and int(np.abs(k).sum()) <= MAX_NON_ONE  # exponent budget: 2^-100 .. 2^100
    k, negative = k.reshape(n, comps), negative.reshape(n, comps)
    exp = np.where(negative.sum(axis=0) & 1, -1.0, 1.0) * 2.0 ** k.sum(axis=0).astype(np.float64)
    return SimpleNamespace(dt=dt, n=n, data=data.astype(npdt), expected=exp.astype(npdt))


# ---- 4: min and max ------------------------------------------------------------------------------------------------
EXTREME_PLACES = ("first", "last", "tail")
FLOAT_VARIANTS = ("plain", "losing_inf", "winning_inf", "zeros")


def extreme_index(dt, n, place):
    """Element that holds the extreme.  "tail": the first element that a loop over whole 16-byte vectors leaves over (the last
    element where nothing is left over or the type fills a vector)."""
    vec = max(1, 16 // elem_bytes(dt))
    if place == "first":
        return 0
    if place == "tail" and n % vec:
        return n - n % vec
    return n - 1


@functools.lru_cache(maxsize=2)
def _magnitudes(size, seed):
    """10^U(0, 30), kept between the places and variants of one case: they differ in a handful of elements."""
    out = 10.0 ** np.random.default_rng(seed).uniform(0, 30, size)
    out.setflags(write=False)
    return out


def extreme_variants(dt):
    return FLOAT_VARIANTS if is_float_kind(dt) else ("plain",)


def extreme_case(dt, n, op, place, seed, variant="plain"):
    """n elements for OP_MIN / OP_MAX where the operator's result is not 0 unless the data hold a zero: max over negative,
    min over positive data (unsigned: positive for both).  Returns a namespace: data (flat), expected (comps values), index.
    Float variants: "plain" finite; "losing_inf" scatters the infinity that must lose; "winning_inf" makes the extreme the
    infinity that must win; "zeros" scatters -0.0 and +0.0, which win over everything else here (the expected 0 compares
    equal to either)."""
    assert op in (OP_MIN, OP_MAX) and place in EXTREME_PLACES and variant in extreme_variants(dt)
    npdt, comps = dtype_info(dt)
    rng = np.random.default_rng(seed)
    at = extreme_index(dt, n, place)
    sign = -1 if (op == OP_MAX and npdt != np.uint32) else 1
    if not is_float_kind(dt):
        if npdt == np.uint32:
            d = rng.integers(1000, 2**32 - 1000, (n, comps), dtype=np.int64)
            best = (2**32 - 1 - np.arange(comps)) if op == OP_MAX else (1 + np.arange(comps))
        else:
            d = sign * rng.integers(1000, 2**31 - 1000, (n, comps), dtype=np.int64)
            best = sign * (1 + np.arange(comps)) if op == OP_MAX else (1 + np.arange(comps))
        d[at] = best
        d = d.astype(npdt)
        return SimpleNamespace(dt=dt, n=n, data=d.reshape(-1), expected=d[at].copy(), index=at)
    # float kinds: magnitudes in [1, 1e30); the extreme is the value nearest to zero
    d = sign * _magnitudes(n * comps, tuple(seed)).reshape(n, comps)
    d[at] = sign * 2.0 ** -(1.0 + np.arange(comps))
    expected = d[at].copy()
    others = np.flatnonzero(np.arange(n) != at)
    some = rng.choice(others, min(others.size, 7), replace=False) if others.size else others
    if variant == "losing_inf":
        d[some] = sign * np.inf
    elif variant == "winning_inf":
        d[at] = -sign * np.inf
        expected = d[at].copy()
    elif variant == "zeros" and some.size:
        d[some] = 0.0
        d[some[::2]] = -0.0
        expected = np.zeros(comps)
    d = d.astype(npdt)
    assert not np.isnan(d).any()
    return SimpleNamespace(dt=dt, n=n, data=d.reshape(-1), expected=expected.astype(npdt), index=at)


# ---- 5: sums that round --------------------------------------------------------------------------------------------
def reference_float(dt):
    """The type the reference sums in: float64 for float components, the 64-bit-mantissa long double for double ones."""
    if mantissa_bits(dt) == 24:
        return np.float64
    assert np.finfo(np.longdouble).nmant >= 63, "the double kinds need a long double wider than double as the reference"
    return np.longdouble


def gamma(k, u):
    """gamma_k = k*u / (1 - k*u), elementwise; needs k*u < 1."""
    ku = np.asarray(k, dtype=np.float64) * u
    assert (ku < 1).all()
    return ku / (1 - ku)


def rounding_data(dt, n, seed):
    """n elements of a float kind: standard normal values times 10^U(-3, 3), so the sign is mixed and small values meet
    large partial sums.  Flat array of n * comps values."""
    assert is_float_kind(dt)
    npdt, comps = dtype_info(dt)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n * comps) * 10.0 ** rng.uniform(-3, 3, n * comps)).astype(npdt)


REFERENCE_BLOCK = 128


def _blocked_cumsum(x):
    """Inclusive cumsum of x (parts x count x comps) along axis 1 in x's own precision with few additions per value: inside
    blocks of REFERENCE_BLOCK elements, plus the running total of the blocks in front: at most REFERENCE_BLOCK - 1 +
    count / REFERENCE_BLOCK + 1 additions instead of count - 1."""
    parts, count, comps = x.shape
    blocks = -(-count // REFERENCE_BLOCK)
    padded = np.zeros((parts, blocks * REFERENCE_BLOCK, comps), dtype=x.dtype)
    padded[:, :count] = x
    inner = np.cumsum(padded.reshape(parts, blocks, REFERENCE_BLOCK, comps), axis=2)
    before = np.zeros((parts, blocks, 1, comps), dtype=x.dtype)
    before[:, 1:, 0] = np.cumsum(inner[:, :-1, -1], axis=1)
    return (inner + before).reshape(parts, -1, comps)[:, :count]


def _tree_sum(x):
    """Sum of x (n x comps) over axis 0 in x's own precision as a balanced tree: ceil(log2 n) additions per value."""
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = np.concatenate([x, np.zeros((1, x.shape[1]), dtype=x.dtype)])
        x = x[0::2] + x[1::2]
    return x[0]


def reference_additions(k, scan):
    """Upper limit of the additions behind one value of the references below that sums k numbers."""
    k = max(int(k), 1)
    return REFERENCE_BLOCK - 1 + -(-k // REFERENCE_BLOCK) + 1 if scan else (k - 1).bit_length()


def rounding_sum_reference(dt, data):
    """(reference sum, bound) per component for the sum of all elements: |result - reference| <= bound for every correct sum."""
    comps = dtype_info(dt)[1]
    x = np.asarray(data).reshape(-1, comps).astype(reference_float(dt))
    return _tree_sum(x), gamma(x.shape[0], unit_roundoff(dt)) * _tree_sum(np.abs(x))


def rounding_scan_reference(dt, data, count, parts):
    """(reference, bound), flat like data, for the exclusive scan: element i of a partition sums i numbers, so its bound is
    gamma_i * sum(|x_j|, j < i), which is 0 for element 0."""
    comps = dtype_info(dt)[1]
    x = np.asarray(data).reshape(parts, count, comps).astype(reference_float(dt))
    ref, mass = np.zeros_like(x), np.zeros_like(x)      # element 0 must be exactly 0
    ref[:, 1:] = _blocked_cumsum(x)[:, :-1]             # (not inclusive - x: that would round once more)
    mass[:, 1:] = _blocked_cumsum(np.abs(x))[:, :-1]
    g = gamma(np.arange(count), unit_roundoff(dt)).reshape(1, count, 1)
    return ref.reshape(-1), (g * mass).reshape(-1)


def within_bound(got, ref, bound):
    """Elementwise |got - ref| <= bound, the difference taken in the reference's precision."""
    return np.abs(np.asarray(got).astype(ref.dtype) - ref) <= bound


# ---- the shapes the GPU tests run (tests/test_gpu_scan_reduce_types.py); tests/test_exact_inputs.py checks the generators on them
def scan_chunk(dt):
    """Elements of one chunk of the reduce-then-scan kernels, as ScanCfg derives it: 256 threads x 4 groups x the elements of a
    16-byte vector."""
    return 256 * 4 * max(1, 16 // elem_bytes(dt))


def scan_wave_elems(dt):
    """Elements one wave takes of a chunk (ScanCfg::WAVE_ELEMS: 64 lanes x 4 groups x the elements of a 16-byte vector): 1024
    for the 4-byte, 512 for the 8-byte, 256 for the 16- and 32-byte types."""
    return 64 * 4 * max(1, 16 // elem_bytes(dt))


def takes_small_partitions_kernel(dt, count, parts):
    """The host's condition for scan_small_partitions_kernel (scan_level in glu_scan_reduce.hip)."""
    return parts >= 2 and count <= scan_wave_elems(dt) and count & (count - 1) == 0 and parts * count > scan_chunk(dt)


def small_partition_shapes(dt):
    """(count, partitions) that take the small-partitions kernel: 256 x 67 for every width (a partition is a whole number
    of groups, or one group, or a quarter of one), 512 x 37 where a wave spans 512 elements or more (the 4- and 8-byte types:
    a partition of several groups)."""
    return ((256, 67), (512, 37)) if elem_bytes(dt) <= 8 else ((256, 67),)


def two_level_count(dt):
    """Smallest count whose chunk sums span several chunks themselves."""
    return scan_chunk(dt) ** 2 + 1


SCAN_POW2_SHAPES = ((8192, 3), (2048, 37))
SCAN_WIDE_COUNTS = (3, 2049, 4097)                  # x 3 partitions
CHAINED_SHAPES = ((32768 * 3 + 5, 2), (32768 * 64, 1))
ROUNDING_SCAN_SHAPE = (8193, 3)
REDUCE_OFFSET_SIZES = (1, 5, 1000, 262147, 3000001)
REDUCE_DOUBLE_SIZES = (7, 4099, 262147, 3000001)
REDUCE_NEUTRAL_SIZES = (1, 3, 255, 1027, 262147)
REDUCE_ROUNDING_SIZES = (262147, 3000001)
REDUCE_TWO_STAGE_SIZE = 300000


def two_level_partitions(dt):
    return (1, 2) if elem_bytes(dt) == 8 else (1,)


def exact_sum_shapes(dt):
    """Every (n, neg) that the GPU tests hand to exact_sums for the float kind dt (n = count x partitions)."""
    shapes = [(c * p, 0.5) for c, p in SCAN_POW2_SHAPES + small_partition_shapes(dt)]
    shapes += [(two_level_count(dt) * p, 0.5) for p in two_level_partitions(dt)]
    if elem_bytes(dt) >= 8:
        shapes += [(c * 3, 0.5) for c in SCAN_WIDE_COUNTS]
    if dt == 0:
        shapes += [(c * p, neg) for c, p in CHAINED_SHAPES for neg in (0.5, 0.0)]
    if elem_bytes(dt) <= 8:
        shapes += [(n, 0.5) for n in REDUCE_OFFSET_SIZES]
    if dt in DOUBLE_KINDS:
        shapes += [(n, 0.5) for n in REDUCE_DOUBLE_SIZES]
    shapes += [(REDUCE_TWO_STAGE_SIZE, 0.5)]
    return shapes


def seed_of(dt, n, tag=0):
    """The seed every user of a case agrees on."""
    return (int(dt), int(n), int(tag))
