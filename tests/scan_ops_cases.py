"""Inputs and expected values of the batched scan with an operator and a kind (glu_scan_run_batch_offsets_op_ptr), without a GPU:
tests/test_scan_ops_cases.py checks this file, tests/test_gpu_scan_ops.py uses it.

Inputs are drawn so that every result is exact in the element type IN ANY GROUPING of the operands, so `==` is the check for
every type and operator whatever a kernel's order of combination is:
  sum   floats k x 0.125 with length x max|k| < 2^24 inside every segment (the rule of tests/test_gpu_batched_scan.py); integers
        are random words and wrap modulo 2^32
  min   values from a small pool (many ties): finite floats of every magnitude and both zeros, or random words.  Which of two
  max   zeros of different sign comes out depends on the grouping, so floats are compared by value there (same_values)
  mul   floats +-2^e with the running sum of the exponents inside [-30, 30] from a segment's first element on: every contiguous
        sub-product then has an exponent inside [-60, 60] and is exact in float32.  The chunk products of the long class come
        from the batched reduce's chunk kernel, where a lane folds every 256th pack of a chunk: products of elements that are NOT
        contiguous.  So the exponents also satisfy sum |e| <= 100 over a segment (most factors are +-1, the signs are random
        everywhere): the product of ANY subset of a segment then lies inside 2^-100 .. 2^100, a normal float32.  Integers are odd
        random words, so that no product collapses to 0
"""
from fractions import Fraction

import numpy as np

import oracle as O

OPS = ("sum", "mul", "min", "max")  # glu_reduce_operator 0 .. 3
MUL_PREFIX_EXPONENT = 30
MUL_TOTAL_EXPONENT = 100


def dtype_info(dt):
    return O.dtype_info(dt)


def is_float(npdt):
    return np.issubdtype(npdt, np.floating)


def identity(op, npdt):
    """The identity of `op` in the scalar type: what an exclusive scan stores first (the batched reduce's identity_of)."""
    if op == "sum":
        return npdt(0)
    if op == "mul":
        return npdt(1)
    if is_float(npdt):
        return npdt(np.inf) if op == "min" else npdt(-np.inf)
    info = np.iinfo(npdt)
    return npdt(info.max) if op == "min" else npdt(info.min)


def make_data(rng, dt, op, offsets, total):
    """total * components scalars of the type of `dt` for a scan with `op` over the segments of `offsets` (see the head)."""
    npdt, comps = dtype_info(dt)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    n = total * comps
    if op == "sum":
        if not is_float(npdt):
            return rng.integers(0, 2**32, n, dtype=np.uint32).view(npdt)
        kmax = np.minimum(4000, ((1 << 24) - 1) // np.maximum(lens, 1))
        per_elem = np.full(total, 4000, dtype=np.int64)
        per_elem[offsets[0]:offsets[-1]] = np.repeat(kmax, lens)
        per_scalar = np.repeat(per_elem, comps)
        k = np.floor(rng.random(n) * (2 * per_scalar + 1)).astype(np.int64) - per_scalar
        return (k * 0.125).astype(npdt)
    if op in ("min", "max"):
        if is_float(npdt):
            pool = np.concatenate([[0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1.0e-38, -1.0e-38],
                                   rng.standard_normal(24) * 10.0 ** rng.integers(-20, 21, 24)]).astype(npdt)
        else:
            pool = rng.integers(0, 2**32, 32, dtype=np.uint32).view(npdt)
        return pool[rng.integers(0, pool.size, n)]
    if not is_float(npdt):
        return (rng.integers(0, 2**32, n, dtype=np.uint32) | np.uint32(1)).view(npdt)
    # per segment and component: up to MUL_TOTAL_EXPONENT steps of +-1 at random places, turned round where the running sum
    # would leave [-MUL_PREFIX_EXPONENT, MUL_PREFIX_EXPONENT]; every other exponent is 0
    exps = np.zeros((total, comps), dtype=np.int64)
    for b, length in zip(offsets[:-1][lens > 0], lens[lens > 0]):
        for c in range(comps):
            at = np.sort(rng.choice(length, min(int(length), MUL_TOTAL_EXPONENT), replace=False))
            steps = rng.choice([-1, 1], at.size)
            run = 0
            for i in range(at.size):
                if abs(run + steps[i]) > MUL_PREFIX_EXPONENT:
                    steps[i] = -steps[i]
                run += steps[i]
            exps[b + at, c] = steps
    sign = np.where(rng.integers(0, 2, (total, comps)) == 1, -1.0, 1.0)
    return (sign * np.exp2(exps.astype(np.float64))).astype(npdt).reshape(-1)


def _accumulate(op, wide):
    fn = {"sum": np.add, "mul": np.multiply, "min": np.minimum, "max": np.maximum}[op]
    return fn.accumulate(wide, axis=0)


def expected(d, dt, op, inclusive, offsets, base=None):
    """`base` (d itself if None: in place) with every segment of `offsets` replaced by the scan of that segment of d, one segment
    at a time: numpy's accumulate in a wide type (float64; uint64 for sums and products, which wrap modulo 2^64 and so are exact
    modulo 2^32; int64 of the values for min and max), then back to the element type."""
    npdt, comps = dtype_info(dt)
    rows = np.asarray(d).reshape(-1, comps)
    out = (rows if base is None else np.asarray(base).reshape(-1, comps)).copy()
    ident = identity(op, npdt)
    for b, e in zip(offsets[:-1], offsets[1:]):
        b, e = int(b), int(e)
        if e <= b:
            continue
        x = rows[b:e]
        if is_float(npdt):
            incl = _accumulate(op, x.astype(np.float64)).astype(npdt)
        elif op in ("sum", "mul"):
            incl = (_accumulate(op, x.view(np.uint32).astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(npdt)
        else:
            incl = _accumulate(op, x.astype(np.int64)).astype(npdt)
        if inclusive:
            out[b:e] = incl
        else:
            out[b] = ident
            out[b + 1:e] = incl[:-1]
    return out.reshape(-1)


def expected_by_loop(d, dt, op, inclusive, offsets):
    """The same by a plain loop over Python numbers (exact: fractions for floats, integers modulo 2^32), for small cases."""
    npdt, comps = dtype_info(dt)
    rows = np.asarray(d).reshape(-1, comps)
    out = rows.copy()
    signed = npdt == np.int32

    def to_py(v):
        return Fraction(float(v)) if is_float(npdt) else int(v)

    def back(v):
        if is_float(npdt):
            return npdt(float(v))
        v &= 0xFFFFFFFF
        return npdt(v - (1 << 32) if signed and v >> 31 else v)

    for b, e in zip(offsets[:-1], offsets[1:]):
        for c in range(comps):
            acc = None  # the identity
            for i in range(int(b), int(e)):
                x = to_py(rows[i, c])
                before = acc
                if acc is None:
                    acc = x
                elif op == "sum":
                    acc = acc + x
                elif op == "mul":
                    acc = acc * x
                elif op == "min":
                    acc = min(acc, x)
                else:
                    acc = max(acc, x)
                if not is_float(npdt) and op in ("sum", "mul"):
                    acc &= 0xFFFFFFFF
                if inclusive:
                    out[i, c] = back(acc)
                else:
                    out[i, c] = identity(op, npdt) if before is None else back(before)
    return out.reshape(-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def same_values(a, b):
    """Equal bit for bit, or equal as numbers (+0.0 and -0.0): the check of float min / max.  A NaN (the poison around and between
    the segments) only equals itself bit for bit."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    bits = (a.view(np.uint8).reshape(a.size, -1) == b.view(np.uint8).reshape(b.size, -1)).all(1)
    with np.errstate(invalid="ignore"):
        return bool((bits | (a.reshape(-1) == b.reshape(-1))).all())


def same(op, npdt, a, b):
    return same_values(a, b) if op in ("min", "max") and is_float(npdt) else same_bits(a, b)


def first_difference(got, want, comps):
    """Index of the first element whose bytes differ, or None."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, got.itemsize * comps)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, want.itemsize * comps)
    bad = np.nonzero((g != w).any(1))[0]
    return int(bad[0]) if bad.size else None


def boundary_lengths(wave, block, chunk, tile):
    """The segment lengths at which the kernels take another path: 0, 1, the limits of the 4-lane and 16-lane groups (a lane
    holds the same number of elements in every group, so they are wave / 16 and wave / 4) and of the wave, the tile of the
    workgroup's loop, the workgroup class's limit, each with the length behind it (the tile also with the one in front), and a
    long segment of three chunks and one element."""
    lens = [0, 1, 2]
    for limit in (wave // 16, wave // 4, wave):
        lens += [limit, limit + 1]
    lens += [tile - 1, tile, tile + 1, block, block + 1, 3 * chunk + 1]
    return lens


def with_empty_between(lens):
    """Two empty segments between each two of `lens`."""
    out = []
    for n in lens:
        out += [n, 0, 0]
    return out[:-2]
