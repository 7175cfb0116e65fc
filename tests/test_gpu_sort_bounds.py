"""GPU tests that no sort call writes outside its arrays, at any alignment: the single sort on every kernel family (one workgroup, the
mid-size kernels, the 128-byte-line scatter and what it falls back to, planned sorts with paired passes and the in-LDS ending, typed
keys and bit ranges), partition_ptr, the segmented sort and the batched sort.  Every caller array lies in an allocation of its own, a
chosen number of bytes behind a 16-byte boundary, with 64 KiB of poison in front of and behind it (the idiom of test_gpu_top_k.py);
after the call the poison is intact, the array holds numpy's stable sort bit for bit, and an array that is only read is unchanged.
Reads outside the arrays are not seen by poison and not tested here."""
import functools

import numpy as np
import pytest

import oracle as O
from test_gpu_segmented_sort import expected as seg_expected, source_major_pieces

pytestmark = pytest.mark.gpu
GUARD = 1 << 16  # bytes of poison on either side: more than the largest LDS tile of pairs (9216 x 8 bytes), so that a store one tile
# too far still lands in poison
POISON = 0xA5
SCRUBBED = 0x5A  # what a poison byte in drawn data becomes
N_PLANNED = (1 << 22) + 54321  # the smallest planned size, and the largest array of this file


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


class Array:
    """The bytes of `d` on the device, `shift` bytes behind a 16-byte boundary, inside an allocation that holds poison in front of
    and behind them."""

    def __init__(self, d, shift=0):
        import torch

        d = np.ascontiguousarray(d)
        self.dtype, self.n, self.nbytes, self.front = d.dtype, d.size, d.nbytes, GUARD + shift
        host = np.concatenate([np.full(self.front, POISON, dtype=np.uint8), d.view(np.uint8).ravel(), np.full(GUARD, POISON, dtype=np.uint8)])
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.front

    @classmethod
    def poisoned(cls, nbytes, shift=0):
        return cls(np.full(nbytes, POISON, dtype=np.uint8), shift)

    def result(self, dtype=None):
        """The array after the call; asserts that the poison around it is intact."""
        raw = self.t.cpu().numpy()
        before, behind = np.flatnonzero(raw[:self.front] != POISON), np.flatnonzero(raw[self.front + self.nbytes:] != POISON)
        assert before.size == 0, "the call wrote in front of the array: %d bytes, from %d to %d bytes before its first" % (
            before.size, self.front - before[0], self.front - before[-1])
        assert behind.size == 0, "the call wrote behind the array: %d bytes, from %d to %d bytes past its end" % (
            behind.size, behind[0], behind[-1])
        return raw[self.front:self.front + self.nbytes].copy().view(dtype or self.dtype)

    def expect(self, want, what):
        """Guards intact and the array equal to `want`, bit for bit."""
        want = bits_of(np.ascontiguousarray(want))
        got = self.result(want.dtype)
        assert got.size == want.size and (got == want).all(), "%s differ at %s" % (what, np.flatnonzero(got != want)[:5])


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch

    torch.cuda.synchronize()


def bits_of(a):
    return a.view("uint%d" % (8 * a.dtype.itemsize))


def scrub(a):
    """A copy of `a` in which no byte is the poison byte."""
    a = np.ascontiguousarray(a).copy()
    b = a.view(np.uint8)
    b[b == POISON] = SCRUBBED
    return a


def no_poison(*arrays):
    """The poison byte occurs in no key and no value of the case: a position the call did not write cannot pass for a result."""
    for a in arrays:
        assert not (np.ascontiguousarray(a).view(np.uint8) == POISON).any(), "the case's data holds the poison byte"


@functools.lru_cache(maxsize=1)
def _iota():
    """The first N_PLANNED uint32 without a poison byte, ascending (the digits of i to the base 255, stepping over the poison): the
    values of every case.  They stand for an iota -- value i is the i-th smallest -- so the stable result is unique."""
    i = np.arange(N_PLANNED, dtype=np.uint32)
    out = np.zeros(N_PLANNED, dtype=np.uint32)
    for byte in range(4):
        d = i % np.uint32(255)
        out |= (d + (d >= POISON)) << np.uint32(8 * byte)
        i //= np.uint32(255)
    assert (np.diff(out.astype(np.int64)) > 0).all()
    out.setflags(write=False)
    return out


def iota(n):
    return _iota()[:n]


def encode(keys):
    """The unsigned integers whose order is the sort's order of `keys` (floats: -0 < +0, NaNs beyond the infinities of their sign): as in
    test_gpu_batched_sort.py."""
    bits = keys.dtype.itemsize * 8
    u = keys.view(np.uint32 if bits == 32 else np.uint64)
    sign = u.dtype.type(1 << (bits - 1))
    if keys.dtype.kind == "u":
        return u
    if keys.dtype.kind == "i":
        return u ^ sign
    return np.where(u & sign, ~u, u | sign)


def decode(code, dtype):
    """The keys of `dtype` whose encode() is `code`."""
    dt = np.dtype(dtype)
    sign = code.dtype.type(1 << (8 * dt.itemsize - 1))
    if dt.kind == "u":
        return code.copy().view(dt)
    if dt.kind == "i":
        return (code ^ sign).view(dt)
    return np.where(code & sign, code ^ sign, ~code).view(dt)


def stable_order(keys, begin_bit=0, end_bit=None):
    """numpy's stable argsort by the bits [begin_bit, end_bit) of the keys' unsigned order."""
    code = encode(keys)
    width = 8 * code.dtype.itemsize
    end_bit = width if end_bit is None else end_bit
    u = code.dtype.type
    if end_bit - begin_bit < width:
        code = (code >> u(begin_bit)) & u((1 << (end_bit - begin_bit)) - 1)
    return np.argsort(code, kind="stable")


def sort_in_place(keys, order, place, call, with_vals=True):
    """One in-place sort of `keys` (and an iota) placed at the byte shifts `place` = (keys, values): guards intact, both arrays equal to
    the expected permutation `order` of the input (None: the call must write nothing)."""
    kshift, vshift = place
    vals = iota(keys.size)
    no_poison(keys, vals)
    ka = Array(keys, kshift)
    va = Array(vals, vshift) if with_vals else None
    assert ka.ptr % 16 == kshift and (va is None or va.ptr % 16 == vshift)
    sync()
    call(ka.ptr, va.ptr if with_vals else None)
    sync()
    ka.expect(keys if order is None else keys[order], "keys")
    if with_vals:
        va.expect(vals if order is None else vals[order], "values")


# the byte shifts (keys, values) of a case: the keys alone, the values alone, both (the line kernel's gate ORs all pointers); 8-byte keys
# stay aligned to their size, their values take every shift
PAIRS_4 = [(0, 0), (4, 0), (8, 0), (12, 0), (0, 4), (0, 8), (0, 12), (4, 4), (8, 8), (12, 12)]
PAIRS_8 = [(0, 0), (8, 0), (0, 4), (0, 8), (0, 12), (8, 4), (8, 8), (8, 12)]
KEYS_4 = [(0, None), (4, None), (8, None), (12, None)]
KEYS_8 = [(0, None), (8, None)]


def places(key_bytes, with_vals):
    return (PAIRS_4 if key_bytes == 4 else PAIRS_8) if with_vals else (KEYS_4 if key_bytes == 4 else KEYS_8)


def place_id(place):
    return "k%d" % place[0] + ("" if place[1] is None else "v%d" % place[1])


def aligned(place):
    return place[0] == 0 and not place[1]


def kind_id(key_bytes, with_vals):
    return "u%d%s" % (8 * key_bytes, "pairs" if with_vals else "keys")


def profiled(G, digit_bits=None, **options):
    s = G.RadixSort(digit_bits=digit_bits, options=options)
    s.set_profiling(True)
    return s


def digit_passes(begin_bit, end_bit, key_bytes, digit_bits):
    """How many counting passes the sort makes over these bits (a digit of an 8-byte key stays inside one 32-bit word)."""
    passes, at = 0, begin_bit
    while at < end_bit:
        bits = min(digit_bits, end_bit - at)
        if key_bytes == 8 and at < 32 < at + bits:
            bits = 32 - at
        at += bits
        passes += 1
    return passes


@functools.lru_cache(maxsize=4)
def uniform_keys(key_bytes, n, seed=0):
    """Uniform keys with duplicates (every fifth is the first)."""
    rng = np.random.default_rng(1000 * key_bytes + n + seed)
    keys = scrub(rng.integers(0, 2**(8 * key_bytes), n, dtype="uint%d" % (8 * key_bytes)))
    keys[::5] = keys[0]
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=8)
def uniform_order(key_bytes, n, end_bit=None):
    return stable_order(uniform_keys(key_bytes, n), 0, end_bit)


def untyped_call(sorter, n, key_bytes, with_vals, num_steps=0):
    if with_vals:
        return lambda k, v: sorter.run_ptr(k, v, n, num_steps, stream(), key_bytes=key_bytes)
    return lambda k, v: sorter.sort_keys_ptr(k, n, num_steps, stream(), key_bytes=key_bytes)


def untyped_cases(counts_4, counts_8, *more):
    """pytest.params (key_bytes, n, with_vals, *more, place) for every count, kind, combination of `more` and placement."""
    out = []
    for key_bytes, counts in ((4, counts_4), (8, counts_8)):
        for n in counts:
            for with_vals in (True, False):
                combos = [()]
                for name, choices in more:
                    combos = [c + ((name, x),) for c in combos for x in choices]
                for combo in combos:
                    for place in places(key_bytes, with_vals):
                        ident = "-".join([kind_id(key_bytes, with_vals), "n%d" % n] + ["%s%d" % nx for nx in combo] + [place_id(place)])
                        out.append(pytest.param(key_bytes, n, with_vals, *[x for _, x in combo], place, id=ident))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. one workgroup


@pytest.mark.parametrize("key_bytes,n,with_vals,steps,place", untyped_cases([2, 5, 1023, 16383, 16384], [8191, 8192], ("steps", (0, 3))))
def test_single_workgroup(G, key_bytes, n, with_vals, steps, place):
    """Up to 16384 4-byte keys (8192 8-byte keys): one workgroup loads the arrays into LDS and stores them from there."""
    keys = uniform_keys(key_bytes, n)
    sorter = profiled(G)
    sort_in_place(keys, uniform_order(key_bytes, n, 4 * steps or None), place, untyped_call(sorter, n, key_bytes, with_vals, steps), with_vals)
    # the single-workgroup kernel is booked as ONE pass; the kernels behind it would make two (12 bits) or a pass per key byte
    assert sorter.read_profile()["passes"] == 1
    if key_bytes == 4 and with_vals and steps == 0:
        ek, ev = O.stable_sort_pairs(keys, iota(n))
        order = uniform_order(key_bytes, n, None)
        assert (ek == keys[order]).all() and (ev == iota(n)[order]).all()


# ------------------------------------------------------------------------------------------------------------------ 2. mid-size kernels


@pytest.mark.parametrize("key_bytes,n,with_vals,digit,unfused,place",
                         untyped_cases([16385, 70001, 123457], [8193, 70001], ("digit", (8, 4)), ("unfused", (0, 1))))
def test_mid_size_kernels(G, key_bytes, n, with_vals, digit, unfused, place):
    """Count, row scan (or the scatter's own prologue) and the small-geometry scatter; the counts are no multiples of 4 or 32: the last
    pack and the last line are partial."""
    keys = uniform_keys(key_bytes, n)
    sorter = profiled(G, digit_bits=digit, SORT_NO_FUSED_SCAN=unfused)
    sort_in_place(keys, uniform_order(key_bytes, n), place, untyped_call(sorter, n, key_bytes, with_vals), with_vals)
    # a pass per digit: not the single workgroup.  No report separates the fused row scan from the launched one, nor the small geometry
    # from the large one: the first is this object's option, the second follows from the count (below every large-tile threshold).
    assert sorter.read_profile()["passes"] == 8 * key_bytes // digit
    if key_bytes == 4 and with_vals and aligned(place):
        ek, ev = O.stable_sort_pairs(keys, iota(n))
        order = uniform_order(key_bytes, n)
        assert (ek == keys[order]).all() and (ev == iota(n)[order]).all()


# ------------------------------------------------------------------------------------------------------------------ 3. line scatter


@pytest.mark.parametrize("key_bytes,n,with_vals,digit,place", untyped_cases([30001, 123457], [30001, 123457], ("digit", (8, 4))))
def test_line_scatter_at_small_sizes(G, key_bytes, n, with_vals, digit, place):
    """SORT_LARGE_MIN=1: every input of at least a tile runs the 128-byte-line scatter -- one to a dozen workgroups, a partial tile behind
    the full ones -- if all its arrays are 16-byte aligned (shift 0), and the large-tile kernel it falls back to if one is not."""
    keys = uniform_keys(key_bytes, n)
    sorter = profiled(G, digit_bits=digit, SORT_LARGE_MIN=1)
    sort_in_place(keys, uniform_order(key_bytes, n), place, untyped_call(sorter, n, key_bytes, with_vals), with_vals)
    # No report separates the line kernel from its fall-back below the planned size (read_plan's pair roles need 2^22 elements): which
    # of the two runs is lines_applicable's test of the four pointers, i.e. this case's placement.
    assert sorter.read_profile()["passes"] == 8 * key_bytes // digit
    if key_bytes == 4 and with_vals and aligned(place):
        ek, ev = O.stable_sort_pairs(keys, iota(n))
        order = uniform_order(key_bytes, n)
        assert (ek == keys[order]).all() and (ev == iota(n)[order]).all()


# ------------------------------------------------------------------------------------------------------------------ 4. planned sorts

CAP_SMALL = 1536  # the in-LDS pass's tile for uniform keys of N_PLANNED: 256 threads x 6 pairs
LONG_RUNS = {"two_long_runs": [(0x1234, 4608 + 5000), (0x4321, 150_000)]}
PLANNED_DTYPE = {"u32pairs": "uint32", "u32keys": "uint32", "u64pairs": "uint64", "int32": "int32", "float32": "float32", "float64": "float64"}


@functools.lru_cache(maxsize=2)
def planned_case(shape, kind):
    """(keys, expected order, expected report) of a shape of test_gpu_lds_finish.py for a kind of key; drawn as the keys' unsigned
    order code, so that the runs of equal top 16 bits are what the shape says for every kind."""
    dt = np.dtype(PLANNED_DTYPE[kind])
    u = np.dtype("uint%d" % (8 * dt.itemsize))
    width, n = 8 * dt.itemsize, N_PLANNED
    rng = np.random.default_rng(len(shape) * 100 + len(kind))
    code = rng.integers(0, 2**width, n, dtype=u)
    want = {"accepted": 1}
    if shape == "range20":  # the device finds bit 20 the top one that varies and takes the runs from bits [4, 20)
        code >>= u.type(width - 20)
        want["top_bit"] = 20
    elif shape == "two_long_runs":  # longer than every enqueued tile (4608): the segmented long-run passes take them
        taken = np.zeros(n, dtype=bool)
        for run, length in LONG_RUNS[shape]:
            pos = rng.choice(np.flatnonzero(~taken), size=length, replace=False)
            code[pos] = (u.type(run) << u.type(width - 16)) | (code[pos] & u.type((1 << (width - 16)) - 1))
            taken[pos] = True
    elif shape == "few17":  # 17 distinct keys: every run is a long run of one key value
        code = rng.integers(0, 2**width, 17, dtype=u)[rng.integers(0, 17, n)]
    elif shape == "all_equal":  # refused: the ordinary passes (all of them identities) run
        code[:] = 0xDEADBEEF
        want["accepted"] = 0
    elif shape == "zeros10":  # a tenth of the keys are zero: one long run of one value, whose 16-bit counters wrap
        code[rng.random(n) < 0.1] = 0
    else:
        assert shape == "uniform"
        want["capacity"] = CAP_SMALL
    keys = scrub(decode(code, dt))
    no_poison(keys)
    code = encode(keys)
    lengths = np.bincount((code >> u.type(width - 16)).astype(np.int64), minlength=65536)
    if shape in ("uniform", "two_long_runs", "zeros10"):
        want["longest_run"] = int(lengths.max())
        want["lengths"] = lengths  # (the runs longer than the tile the device chose go to the long-run passes)
    if shape == "two_long_runs":
        assert int((lengths > CAP_SMALL).sum()) == int((lengths > 4608).sum()) == len(LONG_RUNS[shape])  # (longer than every enqueued tile)
    if shape == "zeros10":
        assert lengths.max() > n // 11
    if shape == "few17":
        want["long_pairs"] = n
    keys.setflags(write=False)
    return keys, np.argsort(code, kind="stable"), want


def planned_cases():
    """Every shape and kind at shift 0, where the paired passes, the in-LDS pass and what stands behind it run (20 sorts), and a choice
    of 15 non-zero shifts: under 40 sorts of this size."""
    shapes = ["uniform", "range20", "two_long_runs", "few17", "all_equal", "zeros10"]
    unaligned = {("uniform", "u32pairs"): [(4, 0), (0, 8), (12, 12)], ("uniform", "u32keys"): [(4, None), (12, None)],
                 ("uniform", "u64pairs"): [(8, 4), (0, 12)], ("uniform", "float32"): [(4, 4)], ("uniform", "int32"): [(0, 12)],
                 ("uniform", "float64"): [(8, 0)], ("range20", "u32pairs"): [(8, 4)], ("two_long_runs", "u32pairs"): [(8, 8)],
                 ("few17", "u32pairs"): [(12, 0)], ("all_equal", "u32pairs"): [(4, 12)], ("zeros10", "u32pairs"): [(0, 4)]}
    combos = [(s, k) for s in shapes for k in ("u32pairs", "u32keys")]
    combos += [(s, k) for k in ("u64pairs", "int32", "float32", "float64") for s in ("uniform", "two_long_runs")]
    out = []
    for shape, kind in combos:
        for place in [(0, 0 if kind != "u32keys" else None)] + unaligned.get((shape, kind), []):
            out.append(pytest.param(shape, kind, place, id="%s-%s-%s" % (shape, kind, place_id(place))))
    assert len(out) < 40
    return out


PLANNED_OPTIONS = dict(SORT_PAIR_MIN=1, SORT_FINISH_MIN=1, SORT_LARGE_MIN=1)


def planned_sort(G, sorter, shape, kind, place):
    """One planned sort of planned_case(shape, kind) on `sorter`, an object made by the caller under PLANNED_OPTIONS: arrays, guards
    and reports as test_planned_sorts states them.  Returns (read_finish, read_long_runs, pair roles)."""
    keys, order, want = planned_case(shape, kind)
    key_bytes, with_vals, typed = keys.dtype.itemsize, kind != "u32keys", kind in ("int32", "float32", "float64")
    if typed:
        def call(k, v):
            sorter.sort_typed_ptr(k, v, keys.size, keys.dtype.name, stream())
    else:
        call = untyped_call(sorter, keys.size, key_bytes, with_vals)
    sort_in_place(keys, order, place, call, with_vals)
    fin, lr = sorter.read_finish(), sorter.read_long_runs()
    roles = sorter.read_plan(key_bytes, roles=True)[2]
    if not aligned(place):
        # no attempt to end in LDS and no pass paired: both need the line kernel, which these arrays do not get.  (That the large-tile
        # kernel and not the small one takes its place is SORT_LARGE_MIN's doing: no report separates the two.)
        assert fin["attempted"] == 0 and roles == [0] * key_bytes, (fin, roles)
        return fin, lr, roles
    assert fin["attempted"] == 1 and fin["accepted"] == want["accepted"], fin
    if not typed:  # (a pass that encodes typed keys on load leads no pair: their ordinary passes pair differently)
        assert roles == [1, 2] * (key_bytes // 2), roles
    for name in ("capacity", "top_bit", "longest_run"):
        if name in want:
            assert fin[name] == want[name], (name, fin, want)
    if "lengths" in want:
        long = want["lengths"][want["lengths"] > fin["capacity"]]
        assert lr["runs"] == long.size and lr["pairs"] == int(long.sum()), (lr, fin)
        assert (shape == "uniform") == (long.size == 0)
    if "long_pairs" in want:
        # (few17: every pair lies in a long run of one key value.  No report tells the few-keys kernel from the other long-run passes.)
        assert lr["pairs"] == want["long_pairs"], (lr, want)
    if kind == "u32pairs":
        ek, ev = O.stable_sort_pairs(keys, iota(keys.size))
        assert (ek == keys[order]).all() and (ev == iota(keys.size)[order]).all()
    return fin, lr, roles


@pytest.mark.parametrize("shape,kind,place", planned_cases())
def test_planned_sorts(G, shape, kind, place):
    """2^22 + 54321 elements with SORT_PAIR_MIN=1 and SORT_FINISH_MIN=1 (and SORT_LARGE_MIN=1: keys-only sorts reach the line kernel at
    2^25 keys otherwise, and a sort of unaligned arrays the large-tile kernel at 4.7 M pairs).  Shift 0: two paired top-bit passes of the
    line kernel, then the in-LDS pass in place on the caller's arrays over runs that begin and end at arbitrary elements, with the
    long-run passes and the few-keys kernel behind it -- or, refused, the ordinary paired passes.  Other shifts: the planned sort of the
    ordinary large-tile kernel on the same data."""
    planned_sort(G, G.RadixSort(options=PLANNED_OPTIONS), shape, kind, place)


# ------------------------------------------------------------------------------------------------------------------ 5. typed keys, bit ranges

KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]


def float_specials(dt):
    """Bit patterns of +-0, +-inf, NaNs of both signs with three payloads, the smallest and the largest denormal of both signs, +-max."""
    u = bits_of(np.zeros(1, dtype=dt)).dtype.type
    width, mant = 8 * dt.itemsize, np.finfo(dt).nmant
    sign, man = 1 << (width - 1), (1 << mant) - 1
    exp = (sign - 1) ^ man
    quiet = 1 << (mant - 1)
    half = [0, exp, exp | 1, exp | quiet | 3, exp | man, 1, man, exp - 1]
    return np.array([u(x) for x in half] + [u(x | sign) for x in half])


@functools.lru_cache(maxsize=2)
def typed_case(dtype, n):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(n + KEY_TYPES.index(dtype))
    if dt.kind == "f":
        keys = scrub((rng.standard_normal(n) * 1e3).astype(dt))
        keys[rng.integers(0, n, n // 20)] = dt.type(1.5)  # duplicates
        special = float_specials(dt)
        where = rng.choice(n, size=max(special.size, n // 50), replace=False)  # about 2 %, every special value at least once
        bits_of(keys)[where] = np.concatenate([special, special[rng.integers(0, special.size, where.size - special.size)]])
    else:
        info = np.iinfo(dt)
        keys = scrub(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))
        keys[::7] = 3 if dt.kind == "u" else -3
    no_poison(keys)
    keys.setflags(write=False)
    return keys, stable_order(keys)


def typed_cases():
    out = []
    for dtype in KEY_TYPES:
        for n in (5000, 70001, 300001):
            for with_vals in (True, False):
                for place in places(np.dtype(dtype).itemsize, with_vals):
                    ident = "%s-n%d-%s-%s" % (dtype, n, "pairs" if with_vals else "keys", place_id(place))
                    out.append(pytest.param(dtype, n, with_vals, place, id=ident))
    return out


@pytest.mark.parametrize("dtype,n,with_vals,place", typed_cases())
def test_typed_keys(G, dtype, n, with_vals, place):
    """sort_typed_ptr: the first pass encodes the keys on load, the last decodes them on store.  Floats with +-0, +-inf, NaNs, denormals."""
    keys, order = typed_case(dtype, n)
    key_bytes = keys.dtype.itemsize
    sorter = profiled(G)
    sort_in_place(keys, order, place, lambda k, v: sorter.sort_typed_ptr(k, v, n, dtype, stream()), with_vals)
    assert sorter.read_profile()["passes"] == (1 if n <= 65536 // key_bytes else key_bytes)  # the single workgroup / a pass per key byte
    if dtype == "uint32" and with_vals and aligned(place):
        ek, ev = O.stable_sort_pairs(keys, iota(n))
        assert (ek == keys[order]).all() and (ev == iota(n)[order]).all()
    if keys.dtype.kind == "f":
        # the header's promise: NaNs stand beyond the infinities of their sign
        out = keys[order]
        negative_nan, positive_nan = np.isnan(out) & np.signbit(out), np.isnan(out) & ~np.signbit(out)
        a, b = int(negative_nan.sum()), int(positive_nan.sum())
        assert a >= 3 and b >= 3
        assert negative_nan[:a].all() and out[a] == -np.inf
        assert positive_nan[n - b:].all() and out[n - b - 1] == np.inf
        assert (out[a + 1:n - b] >= out[a:n - b - 1]).all()


def bit_range_cases():
    out = []
    for key_bytes, ranges in ((4, [(8, 20), (31, 32), (13, 13)]), (8, [(13, 47), (32, 64), (40, 40)])):
        for begin, end in ranges:
            for n in (5000, 70001, 300001):
                for with_vals in (True, False):
                    for place in places(key_bytes, with_vals):
                        ident = "%s-bits%dto%d-n%d-%s" % (kind_id(key_bytes, with_vals), begin, end, n, place_id(place))
                        out.append(pytest.param(key_bytes, begin, end, n, with_vals, place, id=ident))
    return out


@pytest.mark.parametrize("key_bytes,begin,end,n,with_vals,place", bit_range_cases())
def test_bit_ranges(G, key_bytes, begin, end, n, with_vals, place):
    """sort_bit_range_ptr: a range inside a word, the top bit alone, a range across the words of an 8-byte key, its high word; and an
    empty range, which must write nothing at all."""
    keys = uniform_keys(key_bytes, n)
    order = stable_order(keys, begin, end) if end > begin else None
    sorter = profiled(G)
    sort_in_place(keys, order, place, lambda k, v: sorter.sort_bit_range_ptr(k, v, n, begin, end, stream(), key_bytes=key_bytes), with_vals)
    passes = digit_passes(begin, end, key_bytes, 8)
    assert sorter.read_profile()["passes"] == (min(passes, 1) if n <= 65536 // key_bytes else passes)


# ------------------------------------------------------------------------------------------------------------------ 6. partition_ptr

# byte shifts of (source keys, source values, destination keys, destination values); the histogram takes the destination keys' shift
PARTITION_PLACES = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 12, 0), (0, 0, 0, 4), (8, 8, 0, 0), (0, 0, 4, 4), (12, 12, 12, 12)]


@functools.lru_cache(maxsize=8)
def partition_order(n, shift, bits):
    digit = ((uniform_keys(4, n) >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64)
    return np.argsort(digit, kind="stable"), np.bincount(digit, minlength=1 << bits).astype(np.uint32)


def partition(G, sorter, n, shift, bits, with_histogram, place):
    """One partition_ptr call on `sorter`, a profiled object made by the caller: destinations, histogram, sources and guards."""
    keys, vals = uniform_keys(4, n), iota(n)
    order, counts = partition_order(n, shift, bits)
    no_poison(keys, vals)
    sk, sv = Array(keys, place[0]), Array(vals, place[1])
    dk, dv = Array.poisoned(4 * n, place[2]), Array.poisoned(4 * n, place[3])
    hist = Array.poisoned(4 << bits, place[2] & 12)
    sync()
    sorter.partition_ptr(sk.ptr, sv.ptr, dk.ptr, dv.ptr, n, shift, bits, hist.ptr if with_histogram else None, stream())
    sync()
    dk.expect(keys[order], "partitioned keys")
    dv.expect(vals[order], "partitioned values")
    sk.expect(keys, "source keys")  # only read: bit-identical
    sv.expect(vals, "source values")
    hist.expect(counts if with_histogram else np.full(1 << bits, 0xA5A5A5A5, dtype=np.uint32), "histogram")
    assert sorter.read_profile()["passes"] == 1


@pytest.mark.parametrize("place", PARTITION_PLACES, ids=lambda p: "shifts%d.%d.%d.%d" % p)
@pytest.mark.parametrize("with_histogram", [True, False], ids=["histogram", "no_histogram"])
@pytest.mark.parametrize("shift,bits", [(24, 8), (13, 5), (31, 1)])
@pytest.mark.parametrize("n", [200003, (1 << 22) + 5])
def test_partition(G, n, shift, bits, with_histogram, place):
    """One counting pass out of place: the sources are only read, the destinations and the digit histogram lie in poison.  (One pass
    with no plan: no report separates the line kernel, which 2^22 + 5 aligned pairs run, from the kernels the other cases run.)"""
    partition(G, profiled(G), n, shift, bits, with_histogram, place)


# ------------------------------------------------------------------------------------------------------------------ 7. segmented sort

SEG_SHAPES = {65535: (3, 7), 65536: (3, 7), 300_000: (8, 32), 700_001: (8, 32)}  # count: (sources, segments)
SEG_PLACES = [("aligned", 0)] + [(which, shift) for which in ("in", "out", "both") for shift in (4, 12)]


@functools.lru_cache(maxsize=2)
def segmented_case(n, key_bits):
    sources, nseg = SEG_SHAPES[n]
    rng = np.random.default_rng(n + key_bits)
    keys = scrub(rng.integers(0, 2**32, n, dtype=np.uint32))
    keys[::5] &= np.uint32(0xFF00FFFF)  # duplicate-heavy middle byte (no poison: 0 is not)
    begin, length, seg = source_major_pieces(rng, n, sources, nseg)
    ek, ev = seg_expected(keys, iota(n), begin, length, seg, nseg, key_bits)
    return keys, begin, length, seg, nseg, ek, ev


def segmented_sort(G, sorter, n, key_bits, place):
    """One run_segments_ptr call of segmented_case(n, key_bits) on `sorter`, an object made by the caller.  Returns read_seg_finish."""
    keys, begin, length, seg, nseg, ek, ev = segmented_case(n, key_bits)
    which, shift = place
    s_in, s_out = (shift if which in ("in", "both") else 0), (shift if which in ("out", "both") else 0)
    no_poison(keys, iota(n), ek, ev)
    ik, iv = Array(keys, s_in), Array(iota(n), s_in)
    ok, ov = Array.poisoned(4 * n, s_out), Array.poisoned(4 * n, s_out)
    sync()
    sorter.run_segments_ptr(ik.ptr, iv.ptr, ok.ptr, ov.ptr, n, begin, length, seg, nseg, key_bits, stream())
    sync()
    ok.expect(ek, "keys")
    ov.expect(ev, "values")
    ik.result()
    iv.result()
    rep = sorter.read_seg_finish()
    if which == "aligned" and n == 700_001 and key_bits:
        assert rep["attempted"] == 1 and rep["accepted"] == 1 and rep["runs"] == nseg * 256, rep
    elif which != "aligned" or n < 65536 or not key_bits:
        # copies and a sort per segment: never an attempt.  (No report separates the copies from the segmented passes of an aligned call
        # of 2^16 or 300 000 elements that makes no attempt; seg_make_plan decides by the count and the four pointers.)
        assert rep["attempted"] == 0, rep
    return rep


@pytest.mark.parametrize("place", SEG_PLACES, ids=lambda p: "%s%d" % p)
@pytest.mark.parametrize("key_bits", [0, 16, 32])
@pytest.mark.parametrize("n", sorted(SEG_SHAPES))
def test_segmented_sort(G, n, key_bits, place):
    """run_segments_ptr with all four arrays in poison: below 2^16 elements (copies and a sort per segment), from 2^16 (segmented
    passes), 700 001 (ending in LDS); and every count with the inputs, the outputs or both 4 and 12 bytes off a 16-byte boundary, which
    takes the copies whatever the count.  The inputs' contents are unspecified afterwards; their guards must hold."""
    segmented_sort(G, G.RadixSort(), n, key_bits, place)


# ------------------------------------------------------------------------------------------------------------------ 8. batched sort

BATCH_LENGTHS = {"wave": [2, 63, 64, 65, 511, 512] * 8, "block": [513, 1000, 4097, 5000], "long": [16385, 20001]}
BATCH_PATH = {"wave": 1, "block": 2, "long": 3}


@pytest.mark.parametrize("key_bytes,place", [(4, (4, 0)), (4, (0, 12)), (4, (4, 4)), (4, (12, 12)), (8, (8, 4)), (8, (8, 12))],
                         ids=lambda p: place_id(p) if isinstance(p, tuple) else "u%d" % (8 * p))
@pytest.mark.parametrize("cls", ["wave", "block", "long"])
def test_batched_sort(G, cls, key_bytes, place):
    """sort_batch_offsets_ptr on shifted arrays, the segments of one class, offsets[0] > 0 and offsets[-1] < total: guards intact, the
    elements in front of and behind the segments untouched, the offsets only read.  Shift 0 is not run: that the elements outside the
    segments of aligned uint32 pairs stay is what test_elements_outside_the_segments_are_not_touched (test_gpu_batched_sort.py) asserts."""
    lens = np.array(BATCH_LENGTHS[cls], dtype=np.int64)
    assert all(G.plan_batch(int(l), key_bytes)[0] == BATCH_PATH[cls] for l in set(lens.tolist()))
    head, tail = 777, 1234
    offsets = (np.concatenate([[0], np.cumsum(lens)]) + head).astype(np.uint32)
    total = int(offsets[-1]) + tail
    keys = uniform_keys(key_bytes, total, seed=len(cls))
    vals = iota(total)
    no_poison(keys, vals)
    ek, ev = keys.copy(), vals.copy()
    for b, e in zip(offsets[:-1], offsets[1:]):
        order = np.argsort(keys[b:e], kind="stable")
        ek[b:e], ev[b:e] = keys[b:e][order], vals[b:e][order]
    ka, va, oa = Array(keys, place[0]), Array(vals, place[1]), Array(offsets)
    sorter = G.RadixSort()
    sync()
    sorter.sort_batch_offsets_ptr(ka.ptr, va.ptr, total, oa.ptr, lens.size, keys.dtype.name, stream())
    sync()
    ka.expect(ek, "keys")  # (the head and the tail are part of the expected arrays, as they were)
    va.expect(ev, "values")
    oa.expect(offsets, "offsets")
    rb = sorter.read_batch()
    assert {c: rb[c] for c in ("wave", "block", "long")} == {c: (lens.size if c == cls else 0) for c in ("wave", "block", "long")}, rb
