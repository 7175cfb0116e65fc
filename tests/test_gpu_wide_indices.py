"""GPU tests of the eight operators that take counts "below 2^32" -- select, key runs, sorted search, merge, histogram, expand, the
batched scan and the batched sort -- on arrays past 2^31 elements, past 4 GiB and at their count limits: where an element index
needs bit 31, a byte offset needs 33 bits and the tile arithmetic comes within one tile of 2^32.

Every array is made on the device in chunks of 2^28 from a closed form of the element index (shifts, a multiplicative hash), and
every expected value is that closed form again or a torch op evaluated in int64 chunk by chunk: nothing of 2^31 elements passes
through the host, and nothing of the library is part of a reference.  All outputs are integers or copies, compared with `==`;
uint32 bit patterns are compared as int64 after `& 0xFFFFFFFF`.  Every array a call writes lies inside a larger allocation with at
least one tile of poison (0xA5 bytes) in front of it and behind it, which must survive the call, as must every entry the contract
leaves alone.  A truncated index or offset lands inside the same array, so the arrays are compared whole, the elements on both sides
of element 2^31 and byte 2^32 among them.  T, the tile, comes from the operator's plan call.  One call per case, on a caller
stream, after `prepare` where there is one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CHUNK = 1 << 28  # elements per step of a fill or a check
GIB = 1 << 30
M32 = 0xFFFFFFFF
POISON = 0xA5
POISON32 = 0xA5A5A5A5
POISON64 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)  # as int64
TEMP = 8 * GIB  # what the chunked fills and checks hold at a time, at most: a few int64 tensors of CHUNK elements


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def need(nbytes):
    """Skips unless `nbytes` (the arrays of the test and TEMP) and 2 GiB more are free."""
    import torch

    nbytes = int(nbytes) + TEMP
    assert nbytes <= 40 * GIB, "no test may need more than 40 GiB"
    if torch.cuda.mem_get_info()[0] < nbytes + 2 * GIB:
        pytest.skip("needs %d GiB of free HBM" % -(-nbytes // GIB))


def release():
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


def s64(x):
    """The int64 with the bits of the unsigned 64-bit x."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def hash32(i):
    """int64 tensor of indices -> int64 tensor of hashed values in [0, 2^32) (products wrap modulo 2^64, the low 32 bits are exact)."""
    h = (i * 0x9E3779B1) & M32
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA77) & M32
    return h ^ (h >> 13)


def hash32_host(i):
    """hash32 for a numpy array of indices."""
    h = (np.asarray(i, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x85EBCA77)) & np.uint64(M32)
    return (h ^ (h >> np.uint64(13))).astype(np.int64)


def hash64(i):
    """int64 tensor of indices -> int64 tensor of hashed 64-bit patterns."""
    h = i * s64(0x9E3779B97F4A7C15)
    h = h ^ ((h >> 31) & 0x1FFFFFFFF)
    h = h * s64(0xBF58476D1CE4E5B9)
    return h ^ ((h >> 29) & 0x7FFFFFFFF)


def u32(t):
    """The uint32 values of an int32 tensor, as int64."""
    import torch

    return t.to(torch.int64) & M32


def chunks(n, step=CHUNK):
    for lo in range(0, n, step):
        yield lo, min(n, lo + step)


def iota(lo, hi):
    import torch

    return torch.arange(lo, hi, dtype=torch.int64, device="cuda")


def fill(view, fn, step=CHUNK):
    """view[i] = fn(i) for a 1-d tensor view, in chunks (int64 values wrap into narrower integer types)."""
    for lo, hi in chunks(view.numel(), step):
        view[lo:hi] = fn(iota(lo, hi)).to(view.dtype)


def round_up(x, to):
    return -(-x // to) * to


class Guarded:
    """`nbytes` bytes on the device, `shift` bytes behind a 16-byte boundary, inside an allocation that holds `guard` bytes (a tile
    or more) of poison in front of and behind them; the bytes themselves start as poison."""

    def __init__(self, nbytes, guard, shift=0):
        import torch

        guard = round_up(max(int(guard), 256), 256)
        self.nbytes, self.front = int(nbytes), guard + shift
        self.raw = torch.empty(self.front + self.nbytes + guard, dtype=torch.uint8, device="cuda")
        self.raw.fill_(POISON)
        assert self.raw.data_ptr() % 16 == 0
        self.ptr = self.raw.data_ptr() + self.front

    def view(self, dtype):
        return self.raw[self.front:self.front + self.nbytes].view(dtype)

    def intact(self):
        """The poison around the array is as it was."""
        return bool((self.raw[:self.front] == POISON).all()) and bool((self.raw[self.front + self.nbytes:] == POISON).all())


def all_poison(view_u8):
    return all(bool((view_u8[lo:hi] == POISON).all()) for lo, hi in chunks(view_u8.numel(), 1 << 30))


def on_stream(call):
    """call(stream handle) on a stream of the caller's, then one synchronise."""
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()


def last_where(pred, hi=1 << 31):
    """The largest c in [0, hi) with pred(c), for a pred that holds up to some c and not beyond."""
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def small_u32(g):
    """A small Guarded array of uint32 on the host, as int64."""
    import torch

    return u32(g.view(torch.int32)).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ select


def test_select_byte_flags_at_the_count_limit(G):
    """2^32 - 1 stencil bytes (4 GiB), the flags form, indices only: the non-zero bytes at known positions -- the first and the last
    element, both sides of element 2^31, both sides of every 64th tile edge, a hashed remainder -- come back in order; max_out one
    below their number leaves the last slot alone while *num_selected counts them all."""
    import torch

    n = (1 << 32) - 1
    T = G.plan_select(n, G.SelectStencil_Byte)[0]
    pos = {0, (1 << 31) - 1, 1 << 31, n - 1}
    for e in range(64 * T, n, 64 * T):
        pos.update((e - 1, e))
    pos.update(int(x) % n for x in hash32_host(np.arange(1000)))
    pos.discard(POISON32)
    pos = np.array(sorted(pos), dtype=np.int64)
    m = pos.size
    need(n + 8 * m)
    st, out, num = Guarded(n, T), Guarded(4 * m, 4 * T), Guarded(4, 256)
    sv, pt = st.view(torch.uint8), torch.from_numpy(pos).cuda()
    sv.zero_()
    sv[pt] = (1 + pt % 255).to(torch.uint8)
    sel = G.Select()
    sel.prepare(n, G.SelectStencil_Byte)
    on_stream(lambda s: sel.run_ptr(st.ptr, n, m - 1, num.ptr, out_indices_ptr=out.ptr, stencil_type=G.SelectStencil_Byte,
                                    op=G.SelectOperator_NE, threshold=None, stream=s))
    got = small_u32(out)
    assert int(small_u32(num)[0]) == m
    bad = np.flatnonzero(got[:m - 1] != pos[:m - 1])
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(pos[bad[0]]))
    assert int(got[m - 1]) == POISON32, "the slot behind max_out was written"
    assert out.intact() and num.intact() and st.intact()
    assert sum(int(sv[lo:hi].count_nonzero()) for lo, hi in chunks(n, 1 << 30)) == m and bool((sv[pt] == (1 + pt % 255).to(torch.uint8)).all())
    del sel, st, out, num, sv, pt
    release()


def test_select_uint_threshold_past_2_31_elements(G):
    """2^31 + T + 5 hashed uint32, GE 2^31 (about half), indices and 4-byte items, the stencil one element off a 16-byte boundary:
    against torch.nonzero per chunk plus a running base.  Indices and ranks with bit 31 set; max_out leaves a tile of slots alone."""
    import torch

    T = G.plan_select(1 << 31, G.SelectStencil_Uint)[0]
    n = (1 << 31) + T + 5
    assert G.plan_select(n, G.SelectStencil_Uint)[0] == T
    need(14 * n)  # (8 n of inputs, about 4 n and less than 6 n of outputs)
    st, items = Guarded(4 * n, 4 * T, shift=4), Guarded(4 * n, 4 * T)
    sv, iv = st.view(torch.int32), items.view(torch.int32)
    fill(sv, hash32)
    fill(iv, lambda i: (i * 7 + 3) & M32)
    m = sum(int((sv[lo:hi] < 0).sum()) for lo, hi in chunks(n))  # (as uint32: >= 2^31)
    assert n // 4 < m < 3 * n // 4
    max_out = m + T
    oi, ox, num = Guarded(4 * max_out, 4 * T), Guarded(4 * max_out, 4 * T), Guarded(4, 256)
    sel = G.Select()
    sel.prepare(n, G.SelectStencil_Uint)
    on_stream(lambda s: sel.run_ptr(st.ptr, n, max_out, num.ptr, out_indices_ptr=ox.ptr, items_ptr=items.ptr, out_items_ptr=oi.ptr,
                                    item_bytes=4, stencil_type=G.SelectStencil_Uint, op=G.SelectOperator_GE, threshold=1 << 31, stream=s))
    assert int(small_u32(num)[0]) == m
    oxv, oiv, r = ox.view(torch.int32), oi.view(torch.int32), 0
    for lo, hi in chunks(n):
        idx = torch.nonzero(sv[lo:hi] < 0).squeeze(1) + lo
        k = idx.numel()
        assert bool((u32(oxv[r:r + k]) == idx).all()), "indices differ from nonzero in the chunk at %d (ranks from %d)" % (lo, r)
        assert bool((u32(oiv[r:r + k]) == ((idx * 7 + 3) & M32)).all()), "items differ in the chunk at %d (ranks from %d)" % (lo, r)
        r += k
        del idx
    assert r == m and bool((oxv[m:] == POISON32 - (1 << 32)).all()) and bool((oiv[m:] == POISON32 - (1 << 32)).all()), "slots behind the selected were written"
    assert ox.intact() and oi.intact() and num.intact() and st.intact() and items.intact()
    del sel, st, items, oi, ox, num, sv, iv, oxv, oiv
    release()


@pytest.mark.parametrize("item_bytes,every", [(32, 1), (32, 3), (16, 1), (16, 3)])
def test_select_wide_items_past_4_gib(G, item_bytes, every):
    """2^32 / item_bytes + T + 5 items of 32 or 16 bytes under a byte stencil: all selected (source and destination offsets cross
    2^32 together, out_items == items bit for bit) or every third (they differ).  The slots behind the selected keep their poison."""
    import torch

    words = item_bytes // 8
    T = G.plan_select(1 << 28, G.SelectStencil_Byte)[0]
    n = (1 << 32) // item_bytes + T + 5
    assert G.plan_select(n, G.SelectStencil_Byte)[0] == T
    need(2 * n * item_bytes + n)
    mul = [3, s64(0x9E3779B97F4A7C15), 5, s64(0xD6E8FEB86659FD93)]
    items, out, st, num = Guarded(n * item_bytes, T * item_bytes), Guarded(n * item_bytes, T * item_bytes), Guarded(n, T, shift=1), Guarded(4, 256)
    iv, ov, sv = items.view(torch.int64).view(n, words), out.view(torch.int64).view(n, words), st.view(torch.uint8)
    step = CHUNK // 8
    for lo, hi in chunks(n, step):
        i = iota(lo, hi)
        for w in range(words):
            iv[lo:hi, w] = i * mul[w] + w
        sv[lo:hi] = (i % every == 0).to(torch.uint8)
    m = -(-n // every)
    sel = G.Select()
    sel.prepare(n, G.SelectStencil_Byte)
    on_stream(lambda s: sel.run_ptr(st.ptr, n, n, num.ptr, items_ptr=items.ptr, out_items_ptr=out.ptr, item_bytes=item_bytes,
                                    stencil_type=G.SelectStencil_Byte, op=G.SelectOperator_NE, threshold=None, stream=s))
    assert int(small_u32(num)[0]) == m
    for lo, hi in chunks(m, step):
        same = ov[lo:hi] == iv[lo * every:(hi - 1) * every + 1:every]
        if not bool(same.all()):
            r = lo + int(torch.nonzero(~same.all(1))[0])
            raise AssertionError("out_items[%d] = %s, items[%d] = %s" % (r, ov[r].tolist(), r * every, iv[r * every].tolist()))
    assert all_poison(out.view(torch.uint8)[m * item_bytes:]), "slots behind the selected were written"
    assert out.intact() and num.intact() and items.intact() and st.intact()
    del sel, items, out, st, num, iv, ov, sv
    release()


# ---------------------------------------------------------------------------------------------------------------- key runs


@pytest.mark.parametrize("limit,shift,base_shift", [(False, 20, 4), (True, 12, 0)])
def test_key_runs_uint32_heads_past_2_31(G, limit, shift, base_shift):
    """uint32 keys i >> shift: at 2^31 + T + 5 keys (one element off a 16-byte boundary) 2049 runs with heads at the multiples of
    2^20, those at and above 2^31 among them; at the limit of 2^32 - 1 keys (16 GiB) 2^20 runs.  max_runs = runs + 8: the tail of
    offsets holds `count`, the tail of unique_keys its poison."""
    import torch

    T = G.plan_key_runs(1 << 31, 32)[0]
    n = (1 << 32) - 1 if limit else (1 << 31) + T + 5
    assert G.plan_key_runs(n, 32)[0] == T
    runs = ((n - 1) >> shift) + 1
    max_runs = runs + 8
    assert runs == (1 << 20 if limit else 2049)
    need(4 * n)
    keys = Guarded(4 * n, 4 * T, shift=base_shift)
    fill(keys.view(torch.int32), lambda i: i >> shift)
    offs, uniq, num = Guarded(4 * (max_runs + 1), 4 * T), Guarded(4 * max_runs, 4 * T), Guarded(4, 256)
    kr = G.KeyRuns()
    kr.prepare(n, 32)
    on_stream(lambda s: kr.run_ptr(keys.ptr, n, offs.ptr, max_runs, num.ptr, unique_keys_ptr=uniq.ptr, key_bits=32, stream=s))
    assert int(small_u32(num)[0]) == runs
    r = np.arange(runs, dtype=np.int64)
    got = small_u32(offs)
    bad = np.flatnonzero(got != np.concatenate([r << shift, np.full(9, n, dtype=np.int64)]))
    assert bad.size == 0, ("offsets", int(bad[0]), int(got[bad[0]]))
    got = small_u32(uniq)
    bad = np.flatnonzero(got != np.concatenate([r, np.full(8, POISON32, dtype=np.int64)]))
    assert bad.size == 0, ("unique_keys", int(bad[0]), int(got[bad[0]]))
    assert offs.intact() and uniq.intact() and num.intact() and keys.intact()
    del kr, keys, offs, uniq, num
    release()


@pytest.mark.parametrize("whole_key", [False, True])
def test_key_runs_uint64_past_4_gib(G, whole_key):
    """2^29 + T + 5 uint64 keys 3 i (4 GiB).  By the bits [20, 64) run r starts at ceil(r 2^20 / 3); by all 64 bits every key is
    its own run, and with max_runs = count the offsets are the iota (2 GiB of them) with `count` behind it, unique_keys the keys."""
    import torch

    T = G.plan_key_runs(1 << 29, 64)[0]
    n = (1 << 29) + T + 5
    assert G.plan_key_runs(n, 64)[0] == T
    runs = n if whole_key else ((3 * (n - 1)) >> 20) + 1
    max_runs = n if whole_key else runs + 8
    need(8 * n + 12 * max_runs)
    keys = Guarded(8 * n, 8 * T)
    kv = keys.view(torch.int64)
    fill(kv, lambda i: i * 3)
    offs, uniq, num = Guarded(4 * (max_runs + 1), 4 * T), Guarded(8 * max_runs, 8 * T), Guarded(4, 256)
    kr = G.KeyRuns()
    kr.prepare(n, 64)
    on_stream(lambda s: kr.run_ptr(keys.ptr, n, offs.ptr, max_runs, num.ptr, unique_keys_ptr=uniq.ptr, key_bits=64,
                                   begin_bit=0 if whole_key else 20, end_bit=64, stream=s))
    assert int(small_u32(num)[0]) == runs
    ov, uv = offs.view(torch.int32), uniq.view(torch.int64)
    if whole_key:
        for lo, hi in chunks(n):
            i = iota(lo, hi)
            assert bool((u32(ov[lo:hi]) == i).all()), "offsets are not the iota in [%d, %d)" % (lo, hi)
            assert bool((uv[lo:hi] == i * 3).all()), "unique_keys are not the keys in [%d, %d)" % (lo, hi)
        assert int(u32(ov[n:])[0]) == n
    else:
        heads = (np.arange(runs, dtype=np.int64) * (1 << 20) + 2) // 3
        got = small_u32(offs)
        bad = np.flatnonzero(got != np.concatenate([heads, np.full(9, n, dtype=np.int64)]))
        assert bad.size == 0, ("offsets", int(bad[0]), int(got[bad[0]]))
        got = uv.cpu().numpy()
        bad = np.flatnonzero(got != np.concatenate([3 * heads, np.full(8, POISON64, dtype=np.int64)]))
        assert bad.size == 0, ("unique_keys", int(bad[0]), int(got[bad[0]]))
    assert offs.intact() and uniq.intact() and num.intact() and keys.intact()
    del kr, keys, offs, uniq, num, kv, ov, uv
    release()


# ----------------------------------------------------------------------------------------------------------- sorted search


def run_search(G, hay, n, key_type, path, needles_t, needle_shift=0, lower=True, upper=True, guard=4096):
    """One prepared call on `path`; returns the Guarded outputs (None where not asked for)."""
    import torch

    m = needles_t.numel()
    es = needles_t.element_size()
    nd = Guarded(m * es, guard, shift=needle_shift)
    nd.view(needles_t.dtype).copy_(needles_t)
    lo_out = Guarded(4 * m, guard) if lower else None
    up_out = Guarded(4 * m, guard) if upper else None
    search = G.SortedSearch()
    search.set_option("PATH", path)
    search.prepare(n, key_type)
    on_stream(lambda s: search.run_ptr(hay.ptr, n, nd.ptr, m, lo_out.ptr if lower else None, up_out.ptr if upper else None,
                                       key_type=key_type, stream=s))
    assert search.last()[0] == path, search.last()
    assert nd.intact() and bool((nd.view(needles_t.dtype) == needles_t).all()), "the call wrote to its needles"
    del search
    return lo_out, up_out


def check_pair_bounds(n, below, not_above, lo_out, up_out):
    """The haystack holds key(j), j = 0 .. ceil(n / 2) - 1, twice each (the last one once if n is odd): with `below` and `not_above`
    the numbers of distinct keys below / not above every needle, the bounds are min(2 below, n) and min(2 not_above, n)."""
    for name, out, distinct in (("lower", lo_out, below), ("upper", up_out, not_above)):
        want = np.minimum(2 * np.asarray(distinct, dtype=np.int64), n)
        got = small_u32(out)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
        assert out.intact()


@pytest.mark.parametrize("limit,path", [(False, "Direct"), (False, "Indexed"), (True, "Indexed")])
def test_sorted_search_uint32_haystack_past_2_31(G, limit, path):
    """Haystack 2 (i >> 1), pairs of equal even keys, of 2^31 + 37 keys and at the limit of 2^32 - 1 keys (16 GiB, the index built
    in the call); 2^16 needles: hashed even and odd ones, 0, the largest key, one beyond it, the keys around element 2^31.  Both
    bounds in closed form, those with bit 31 set among them."""
    import torch

    n = (1 << 32) - 1 if limit else (1 << 31) + 37
    need(4 * n + G.plan_sorted_search(n, 1 << 16)[3])
    hay = Guarded(4 * n, 4096)
    fill(hay.view(torch.int32), lambda i: (i >> 1) << 1)
    distinct = (n + 1) // 2
    top = 2 * (distinct - 1)
    v = hash32_host(np.arange(1 << 16))
    special = [0, 1, 2, top - 1, top, min(top + 1, M32), M32, (1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 2, 1 << 30,
               (1 << 30) - 1]
    v[:len(special)] = special
    needles = torch.from_numpy(v.astype(np.uint32).view(np.int32)).cuda()
    lo_out, up_out = run_search(G, hay, n, "uint32", getattr(G, "SearchPath_" + path), needles)
    check_pair_bounds(n, np.minimum((v + 1) // 2, distinct), np.minimum(v // 2 + 1, distinct), lo_out, up_out)
    assert int(small_u32(lo_out)[9]) == 1 << 31 and int(small_u32(up_out)[9]) == (1 << 31) + 2  # (the needle 2^31)
    assert hay.intact()
    del hay, lo_out, up_out, needles
    release()


@pytest.mark.parametrize("key_type", ["uint64", "float64"])
@pytest.mark.parametrize("path", ["Direct", "Indexed"])
def test_sorted_search_wide_keys_past_4_gib(G, key_type, path):
    """2^29 + 37 eight-byte keys (4 GiB), pairs of equal ones: uint64 keys j (2^33 + 1), so that both words of a key decide, and
    float64 keys (j - 2^27) / 2 with a negative half, so that the order is the sort's.  2^16 needles on and between the keys, beyond
    both ends and around the key at byte 2^32."""
    import torch

    n = (1 << 29) + 37
    need(8 * n + G.plan_sorted_search(n, 1 << 16, key_type)[3])
    hay = Guarded(8 * n, 4096)
    distinct = (n + 1) // 2
    j = hash32_host(np.arange(1 << 16)) % (distinct + 50)
    j[:8] = [0, 1, distinct - 1, distinct, 1 << 27, (1 << 27) - 1, 1 << 28, (1 << 28) - 1]  # (key j is elements 2 j and 2 j + 1)
    d = np.arange(1 << 16, dtype=np.int64) % 3 - 1
    if key_type == "uint64":
        K = (1 << 33) + 1
        fill(hay.view(torch.int64), lambda i: (i >> 1) * K)
        v = [max(0, int(a) * K + int(b)) for a, b in zip(j, d)] + [(1 << 64) - 1, (1 << 63), (1 << 63) - 1]
        below = [min(-(-x // K), distinct) for x in v]
        not_above = [min(x // K + 1, distinct) for x in v]
        needles = torch.from_numpy(np.array(v, dtype=np.uint64).view(np.int64)).cuda()
    else:
        half = 1 << 27
        fill(hay.view(torch.float64), lambda i: ((i >> 1) - half).to(torch.float64) * 0.5)
        k = 2 * (j - half) + d  # needles k / 4 against keys 2 (j - half) / 4
        v = np.concatenate([k * 0.25, [-np.inf, np.inf, -1e300, 1e300]])
        k = np.concatenate([k, [-(1 << 40), 1 << 40, -(1 << 40), 1 << 40]])
        below = np.clip(-(-k // 2) + half, 0, distinct)
        not_above = np.clip(k // 2 + half + 1, 0, distinct)
        needles = torch.from_numpy(v).cuda()
    lo_out, up_out = run_search(G, hay, n, key_type, getattr(G, "SearchPath_" + path), needles)
    check_pair_bounds(n, below, not_above, lo_out, up_out)
    assert hay.intact()
    del hay, lo_out, up_out, needles
    release()


@pytest.mark.parametrize("path,shift", [("Direct", 0), ("Indexed", 8)])
def test_sorted_search_needles_past_4_gib(G, path, shift):
    """2^29 + T + 5 uint64 needles (4 GiB; T the needles of a tile) into 2^20 keys, lower bounds only (2 GiB of them), the needles
    16-byte aligned or one element off: against torch.searchsorted per chunk."""
    import torch

    T = G.SortedSearch.needle_tile("uint64")
    m, n = (1 << 29) + T + 5, 1 << 20
    need(12 * m)
    hay, nd, out = Guarded(8 * n, 4096), Guarded(8 * m, 8 * T, shift=shift), Guarded(4 * m, 4 * T)
    hv, nv, ov = hay.view(torch.int64), nd.view(torch.int64), out.view(torch.int32)
    fill(hv, lambda i: i * 4097)
    fill(nv, lambda i: hash64(i) % (n * 4097 + 5000))
    search = G.SortedSearch()
    search.set_option("PATH", getattr(G, "SearchPath_" + path))
    search.prepare(n, "uint64")
    on_stream(lambda s: search.run_ptr(hay.ptr, n, nd.ptr, m, out.ptr, None, key_type="uint64", stream=s))
    assert search.last()[0] == getattr(G, "SearchPath_" + path)
    for lo, hi in chunks(m):
        want = torch.searchsorted(hv, nv[lo:hi])
        same = u32(ov[lo:hi]) == want
        if not bool(same.all()):
            r = int(torch.nonzero(~same)[0])
            raise AssertionError("out_lower[%d] = %d, searchsorted gives %d" % (lo + r, int(u32(ov[lo + r:lo + r + 1])), int(want[r])))
        del want, same
    assert out.intact() and nd.intact() and hay.intact()
    del search, hay, nd, out, hv, nv, ov
    release()


# ------------------------------------------------------------------------------------------------------------------- merge


@pytest.mark.parametrize("na,nb,shift", [((1 << 31) + 7, (1 << 20) + 3, 11), ((1 << 32) - 1 - (1 << 16), 1 << 16, 16)])
def test_merge_uint32_keys_past_2_31_and_at_the_limit(G, na, nb, shift):
    """A[i] = i, B[j] = j << shift, keys only: past 2^31 outputs, and na + nb = 2^32 - 1 (32 GiB with the output).  The keys of B tie
    with keys of A and come behind them: A[i] lands at i + min(ceil(i / 2^shift), nb), B[j] at j + min((j << shift) + 1, na); the
    two sets of positions are the whole output."""
    import torch

    T = G.plan_merge(na, nb, "uint32", False)[0]
    total = na + nb
    need(4 * (na + nb + total) - TEMP // 2)  # (the checks go by 2^26: half a GiB at a time)
    a, b, out = Guarded(4 * na, 4 * T), Guarded(4 * nb, 4 * T), Guarded(4 * total, 4 * T)
    fill(a.view(torch.int32), lambda i: i, 1 << 26)
    fill(b.view(torch.int32), lambda j: j << shift, 1 << 26)
    merge = G.Merge()
    merge.prepare(total, "uint32")
    on_stream(lambda s: merge.run_ptr(a.ptr, None, na, b.ptr, None, nb, out.ptr, None, key_type="uint32", stream=s))
    assert merge.last() == G.plan_merge(na, nb, "uint32", False)[1:3]
    ov = out.view(torch.int32)
    for lo, hi in chunks(na, 1 << 26):
        i = iota(lo, hi)
        at = i + torch.clamp((i + (1 << shift) - 1) >> shift, max=nb)
        same = u32(ov[at]) == i
        if not bool(same.all()):
            r = int(torch.nonzero(~same)[0])
            raise AssertionError("A[%d] is not at out[%d], which holds %d" % (lo + r, int(at[r]), int(u32(ov[at[r]:at[r] + 1]))))
        del i, at, same
    j = iota(0, nb)
    at = j + torch.clamp((j << shift) + 1, max=na)
    assert bool((u32(ov[at]) == (j << shift)).all()), "a key of B is not where it belongs"
    assert int(at[-1]) == total - 1
    assert out.intact() and a.intact() and b.intact()
    del merge, a, b, out, ov, j, at
    release()


def test_merge_uint64_pairs_past_4_gib(G):
    """na = nb = 2^28 + T / 2 + 3 uint64 keys with values: 2^29 + T + 6 pairs leave, 4 GiB of keys and 2 GiB of values.  Keys in
    long ties, (i >> 10) K in A and (j >> 9) K in B; the values i and 2^31 + j tell the side and the place.  Ascending, every key
    the key of its value's source, A first and in order among equal keys, the values a permutation."""
    import torch

    T = G.plan_merge(1 << 28, 1 << 28, "uint64", True)[0]
    na = nb = (1 << 28) + T // 2 + 3
    total, K = na + nb, (1 << 34) + 3
    assert G.plan_merge(na, nb, "uint64", True)[0] == T
    need(12 * (na + nb + total) + total)
    ak, bk, ok = Guarded(8 * na, 8 * T), Guarded(8 * nb, 8 * T, shift=8), Guarded(8 * total, 8 * T)
    av, bv, ovl = Guarded(4 * na, 4 * T), Guarded(4 * nb, 4 * T, shift=4), Guarded(4 * total, 4 * T)
    fill(ak.view(torch.int64), lambda i: (i >> 10) * K)
    fill(bk.view(torch.int64), lambda j: (j >> 9) * K)
    fill(av.view(torch.int32), lambda i: i)
    fill(bv.view(torch.int32), lambda j: j + (1 << 31))
    merge = G.Merge()
    merge.prepare(total, "uint64")
    on_stream(lambda s: merge.run_ptr(ak.ptr, av.ptr, na, bk.ptr, bv.ptr, nb, ok.ptr, ovl.ptr, key_type="uint64", stream=s))
    gk, gv = ok.view(torch.int64), ovl.view(torch.int32)
    seen = torch.zeros(total, dtype=torch.bool, device="cuda")
    for lo, hi in chunks(total, CHUNK // 2):
        k, v = gk[lo:hi], u32(gv[lo:hi])
        from_b = v >= (1 << 31)
        src = torch.where(from_b, v - (1 << 31), v)
        assert bool((src < torch.where(from_b, nb, na)).all()), "a value that no input holds in [%d, %d)" % (lo, hi)
        assert bool((k == torch.where(from_b, src >> 9, src >> 10) * K).all()), "a key that is not its value's in [%d, %d)" % (lo, hi)
        seen[torch.where(from_b, src + na, src)] = True
        kn, vn = gk[lo + 1:min(total, hi + 1)], u32(gv[lo + 1:min(total, hi + 1)])
        c = kn.numel()
        assert bool((kn >= k[:c]).all()), "keys not ascending in [%d, %d)" % (lo, hi)
        assert bool(((vn > v[:c]) | (kn != k[:c])).all()), "not stable, A first, in [%d, %d)" % (lo, hi)
        del k, v, from_b, src, kn, vn
    assert bool(seen.all()), "the values are no permutation"
    for g in (ak, bk, ok, av, bv, ovl):
        assert g.intact()
    del merge, ak, bk, ok, av, bv, ovl, gk, gv, seen
    release()


# --------------------------------------------------------------------------------------------------------------- histogram


@pytest.mark.parametrize("accumulate", [False, True])
def test_histogram_one_bin_counts_past_2_31(G, accumulate):
    """2^31 + T + 5 equal uint32 samples into 256 even bins: one count with bit 31 set, 255 zeros.  Accumulated on 0xF0000000 + b
    the sums wrap modulo 2^32."""
    import torch

    T = G.plan_histogram(1 << 31, 256)[2]
    n = (1 << 31) + T + 5
    assert G.plan_histogram(n, 256)[2] == T
    need(4 * n)
    x, out = Guarded(4 * n, 4 * T), Guarded(4 * 256, 4 * T)
    x.view(torch.int32).fill_(123456)
    prior = np.arange(256, dtype=np.int64) + 0xF0000000 if accumulate else np.zeros(256, dtype=np.int64)
    if accumulate:
        out.view(torch.int32).copy_(torch.from_numpy(prior.astype(np.uint32).view(np.int32)))
    hist = G.Histogram()
    hist.prepare(n, 256)
    on_stream(lambda s: hist.run_even_ptr(x.ptr, n, 0, 256000, 256, out.ptr, accumulate=accumulate, stream=s))
    want = prior.copy()
    want[123] += n
    assert (small_u32(out) == want & M32).all(), small_u32(out)[120:126]
    assert out.intact() and x.intact()
    del hist, x, out
    release()


@pytest.mark.parametrize("limit,bins,shift", [(False, 8192, 0), (False, 1 << 20, 4), (True, 256, 0)])
def test_histogram_even_bins_of_hashed_uint32(G, limit, bins, shift):
    """Hashed uint32 samples into even bins of width floor((2^32 - 1) / bins), the samples above the last bin dropped: 8192 bins (the
    table in LDS) and 2^20 bins (atomics on the counts, the samples one element off a 16-byte boundary) at 2^31 + T + 5 samples,
    256 bins at the limit of 2^32 - 1 samples (16 GiB).  Against torch.bincount of x // width, summed over the chunks in int64."""
    import torch

    T = G.plan_histogram(1 << 31, bins)[2]
    n = (1 << 32) - 1 if limit else (1 << 31) + T + 5
    path = G.plan_histogram(n, bins)[0]
    assert G.plan_histogram(n, bins)[2] == T and path == (G.HistogramPath_Lds if bins <= 8192 else G.HistogramPath_Global)
    need(4 * n + 12 * bins)
    width = M32 // bins
    hi_edge = bins * width
    x, out = Guarded(4 * n, 4 * T, shift=shift), Guarded(4 * bins, 4 * T)
    xv = x.view(torch.int32)
    fill(xv, hash32)
    hist = G.Histogram()
    hist.prepare(n, bins)
    on_stream(lambda s: hist.run_even_ptr(x.ptr, n, 0, hi_edge, bins, out.ptr, stream=s))
    assert hist.last()[0] == path
    want = torch.zeros(bins, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(n):
        v = u32(xv[lo:hi])
        want += torch.bincount(v[v < hi_edge] // width, minlength=bins)
        del v
    assert int(want.sum()) < n, "no sample was dropped"
    got = u32(out.view(torch.int32))
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert out.intact() and x.intact()
    del hist, x, out, xv, want, got
    release()


def test_histogram_uint64_edges_past_4_gib(G):
    """2^29 + T + 5 hashed uint64 samples (4 GiB) between 257 device edges spread over the unsigned range, samples below the first
    and above the last dropped: against searchsorted and bincount per chunk, with bit 63 flipped so that int64 orders as uint64."""
    import torch

    bins = 256
    T = G.plan_histogram(1 << 29, bins, "uint64", "edges")[2]
    n = (1 << 29) + T + 5
    assert G.plan_histogram(n, bins, "uint64", "edges")[2] == T
    need(8 * n)
    x, out = Guarded(8 * n, 8 * T), Guarded(4 * bins, 4 * T)
    xv = x.view(torch.int64)
    fill(xv, hash64)
    edges = torch.from_numpy(np.array([(k + 3) * ((1 << 64) // 262) for k in range(bins + 1)], dtype=np.uint64).view(np.int64)).cuda()
    flip = -(1 << 63)
    hist = G.Histogram()
    hist.prepare(n, bins)
    on_stream(lambda s: hist.run_edges_ptr(x.ptr, n, edges.data_ptr(), bins, out.ptr, key_type="uint64", stream=s))
    want = torch.zeros(bins, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(n):
        b = torch.searchsorted(edges ^ flip, xv[lo:hi] ^ flip, right=True) - 1
        want += torch.bincount(b[(b >= 0) & (b < bins)], minlength=bins)
        del b
    assert 0 < int(want.sum()) < n and int(want.min()) > 0
    got = u32(out.view(torch.int32))
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert out.intact() and x.intact()
    del hist, x, out, xv, want, got, edges
    release()


def test_histogram_float64_even_bins_past_4_gib(G):
    """2^29 + T + 5 float64 samples k / 4 (4 GiB) into 1024 even bins over [0, 2^18): the scale is 2^-8, so the bin is exactly
    floor(k / 1024); negative samples and samples at or above 2^18 are dropped, and so are a NaN and 1e300 put into the last,
    partial tile, beyond byte 2^32."""
    import torch

    bins, top = 1024, float(1 << 18)
    T = G.plan_histogram(1 << 29, bins, "float64")[2]
    n = (1 << 29) + T + 5
    assert G.plan_histogram(n, bins, "float64")[2] == T
    need(8 * n)
    x, out = Guarded(8 * n, 8 * T), Guarded(4 * bins, 4 * T)
    xv = x.view(torch.float64)
    fill(xv, lambda i: (hash32(i) % ((1 << 20) + 8192) - 4096).to(torch.float64) * 0.25)
    xv[n - 1], xv[n - 2], xv[n - 3] = 1.25, float("nan"), 1e300
    hist = G.Histogram()
    hist.prepare(n, bins)
    on_stream(lambda s: hist.run_even_ptr(x.ptr, n, 0.0, top, bins, out.ptr, key_type="float64", stream=s))
    want = torch.zeros(bins, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(n):
        v = xv[lo:hi]
        v = v[(v >= 0.0) & (v < top)]
        want += torch.bincount((v * (bins / top)).floor().to(torch.int64), minlength=bins)
        del v
    assert 0 < int(want.sum()) <= n - 2
    got = u32(out.view(torch.int32))
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert out.intact() and x.intact()
    del hist, x, out, xv, want, got
    release()


# ------------------------------------------------------------------------------------------------------------------ expand


def offsets_from(start, lengths, end):
    """start, then start + the running sums of `lengths`, none beyond `end` (segments past it are empty)."""
    lengths = np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.int64)) for x in lengths])
    return np.minimum(start + np.concatenate([[0], np.cumsum(lengths)]), end)


def hashed_lengths(count, most, seed):
    """`count` lengths below `most`, every third group of seven of them empty."""
    k = np.arange(count)
    return (hash32_host(k + seed) % most) * ((k // 7) % 3 != 1)


def check_expand(offsets, total, segs=None, ranks=None, items=None, out_items=None, step=CHUNK):
    """Against s(j) = searchsorted(offsets, j, right) - 1 per chunk: the covered positions hold s(j), j - offsets[s(j)] and
    items[s(j)], every other position its poison."""
    import torch

    nseg = offsets.size - 1
    off = torch.from_numpy(offsets).cuda()
    for lo, hi in chunks(total, step):
        j = iota(lo, hi)
        s = torch.searchsorted(off, j, right=True) - 1
        covered = (s >= 0) & (s < nseg)
        s = s.clamp(0, nseg - 1)
        for name, out, want in (("segments", segs, s), ("ranks", ranks, j - off[s])):
            if out is not None:
                same = u32(out[lo:hi]) == torch.where(covered, want, POISON32)
                if not bool(same.all()):
                    r = int(torch.nonzero(~same)[0])
                    raise AssertionError("%s[%d] = %d, segment %d from %d, covered %s" % (name, lo + r, int(u32(out[lo + r:lo + r + 1])), int(s[r]),
                                                                                         int(off[s[r]]), bool(covered[r])))
        if out_items is not None:
            same = (out_items[lo:hi] == torch.where(covered[:, None], items[s], POISON64)).all(1)
            if not bool(same.all()):
                r = int(torch.nonzero(~same)[0])
                raise AssertionError("out_items[%d] = %s, segment %d" % (lo + r, out_items[lo + r].tolist(), int(s[r])))
        del j, s, covered
    del off


@pytest.mark.parametrize("layout", ["long_segment", "start_at_2_31", "cover_from_2_31_minus_3"])
def test_expand_segments_and_ranks_past_2_31(G, layout):
    """total = 2^31 + T + 5, segments and ranks, about 3000 segments of hashed lengths with runs of empty ones, a run longer than a
    merged tile among them.  long_segment: one segment longer than 2^31 (ranks with bit 31 set).  start_at_2_31: a segment that
    starts at exactly 2^31.  cover_from_2_31_minus_3: offsets[0] = 2^31 - 3, everything below keeps its poison.  The cover is
    partial at both ends in all three."""
    import torch

    T = G.plan_expand(1 << 31, 4096)[0]
    total = (1 << 31) + T + 5
    empties = np.zeros(T + 9, dtype=np.int64)
    if layout == "long_segment":
        offsets = offsets_from(11, [hashed_lengths(7, 9, 1), (1 << 31) + 50, 3, empties, hashed_lengths(3000, 3, 2)], total - 7)
        assert offsets[8] - offsets[7] > 1 << 31
    elif layout == "start_at_2_31":
        head = hashed_lengths(1500, 2000, 3)
        offsets = offsets_from(11, [head, (1 << 31) - 11 - int(head.sum()), 40, empties, hashed_lengths(1500, 5, 4)], total - 7)
        assert offsets[1501] == 1 << 31 and offsets[1502] > offsets[1501]
    else:
        offsets = offsets_from((1 << 31) - 3, [hashed_lengths(60, 90, 5), empties, hashed_lengths(60, 90, 6)], total - 2)
    nseg = offsets.size - 1
    assert G.plan_expand(total, nseg)[0] == T and offsets[-1] < total
    need(8 * total)
    off, segs, ranks = Guarded(4 * (nseg + 1), 4 * T), Guarded(4 * total, 4 * T), Guarded(4 * total, 4 * T, shift=4)
    off.view(torch.int32).copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))
    expand = G.Expand()
    expand.prepare(total, nseg)
    on_stream(lambda s: expand.run_ptr(off.ptr, nseg, total, out_segments_ptr=segs.ptr, out_ranks_ptr=ranks.ptr, stream=s))
    assert expand.last() == G.plan_expand(total, nseg)[1:3]
    check_expand(offsets, total, segs.view(torch.int32), ranks.view(torch.int32))
    assert segs.intact() and ranks.intact() and off.intact()
    assert (small_u32(off) == offsets).all(), "the call wrote to its offsets"
    del expand, off, segs, ranks
    release()


@pytest.mark.parametrize("item_bytes", [32, 8])
def test_expand_items_past_4_gib(G, item_bytes):
    """2^16 segments of hashed lengths over 2^32 / item_bytes + T + 5 elements: out_items crosses byte 2^32 (32-byte items at
    2^27 + T + 5, 8-byte items at 2^29 + T + 5), the cover partial at both ends."""
    import torch

    words, nseg = item_bytes // 8, 1 << 16
    T = G.plan_expand(1 << 29, nseg)[0]
    total = (1 << 32) // item_bytes + T + 5
    assert G.plan_expand(total, nseg)[0] == T
    offsets = offsets_from(5, [hashed_lengths(nseg, 3 * total // nseg, 7)], total - 3)
    offsets[-1] = total - 3  # (the last segment takes the rest)
    need(total * item_bytes)
    off, items, out = Guarded(4 * (nseg + 1), 4 * T), Guarded(nseg * item_bytes, 4096), Guarded(total * item_bytes, T * item_bytes)
    off.view(torch.int32).copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))
    iv = items.view(torch.int64).view(nseg, words)
    for w in range(words):
        iv[:, w] = iota(0, nseg) * [s64(0x9E3779B97F4A7C15), 3, s64(0xD6E8FEB86659FD93), 5][w] + w
    expand = G.Expand()
    expand.prepare(total, nseg)
    on_stream(lambda s: expand.run_ptr(off.ptr, nseg, total, items_ptr=items.ptr, out_items_ptr=out.ptr, item_bytes=item_bytes, stream=s))
    check_expand(offsets, total, items=iv, out_items=out.view(torch.int64).view(total, words), step=CHUNK // 8)
    assert out.intact() and items.intact() and off.intact()
    del expand, off, items, out, iv
    release()


def test_expand_segments_at_the_limit(G):
    """total + num_segments + 1 = 2^32 - 1 with 2^16 segments, segments only (16 GiB): the merged diagonal within one tile of 2^32."""
    import torch

    nseg = 1 << 16
    total = (1 << 32) - 2 - nseg
    T = G.plan_expand(total, nseg)[0]
    offsets = offsets_from(0, [hashed_lengths(nseg, 3 * total // nseg, 8)], total)
    offsets[-1] = total
    need(4 * total)
    off, segs = Guarded(4 * (nseg + 1), 4 * T), Guarded(4 * total, 4 * T)
    off.view(torch.int32).copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))
    expand = G.Expand()
    expand.prepare(total, nseg)
    on_stream(lambda s: expand.run_ptr(off.ptr, nseg, total, out_segments_ptr=segs.ptr, stream=s))
    assert expand.last() == G.plan_expand(total, nseg)[1:3]
    check_expand(offsets, total, segs.view(torch.int32))
    assert segs.intact() and off.intact()
    del expand, off, segs
    release()


# ------------------------------------------------------------------------------------------------------------ batched scan


def scan_classes(G, es):
    """The longest segment of the wave class and of the workgroup class for elements of `es` bytes, from plan_scan_batch."""
    return last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 1), last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 2)


def count_classes(path_of, lengths):
    paths = [path_of(int(c)) for c in lengths]
    return {"wave": paths.count(1), "block": paths.count(2), "long": paths.count(3)}


def check_scanned_region(dv, comps, offsets, original):
    """The elements of the segments, [offsets[0], offsets[-1]), against cumsum in int64 per segment, masked to 32 bits."""
    import torch

    b, e = int(offsets[0]), int(offsets[-1])
    lens = torch.from_numpy(np.diff(offsets)).cuda()
    x = original(iota(b * comps, e * comps)).view(e - b, comps)
    excl = torch.cumsum(x, 0, dtype=torch.int64) - x
    seg = torch.repeat_interleave(torch.arange(lens.numel(), device="cuda"), lens)
    starts = torch.from_numpy(offsets[:-1] - b).cuda().clamp(max=e - b - 1)
    want = (excl - excl[starts[seg]]) & M32
    same = (u32(dv[b * comps:e * comps]).view(e - b, comps) == want).all(1)
    if not bool(same.all()):
        r = int(torch.nonzero(~same)[0])
        s = int(seg[r])
        raise AssertionError("element %d, segment %d = [%d, %d)" % (b + r, s, int(offsets[s]), int(offsets[s + 1])))


@pytest.mark.parametrize("layout", ["long_spans", "wave_starts_below"])
@pytest.mark.parametrize("dt,boundary,room", [("Uint", 1 << 31, 1 << 20), ("UVec2", 1 << 29, 1 << 18)])
def test_batched_scan_around_2_31_elements_and_4_gib(G, dt, boundary, room, layout):
    """uint32 around element 2^31 (total 2^31 + 2^20 + 5) and uvec2, 8 bytes, around byte 2^32 (total 2^29 + 2^18 + 5): segments of
    the three classes on both sides of the boundary; a long segment that spans it (long_spans) or a wave-class segment that starts
    one element below it (wave_starts_below, the data one element off a 16-byte boundary).  Everything outside the segments, a tail
    behind the last offset included, is untouched."""
    import torch

    comps = 2 if dt == "UVec2" else 1
    es = 4 * comps
    wave, block = scan_classes(G, es)
    total = boundary + room + 5
    before = [wave, 3, block, wave + 1, 0, 0, 5 * block + 17, 1, block + 1, 0, wave - 1]
    after = [wave, 1, 0, block, 7 * block + 3, wave + 1, 33, 0, block + 1, 2]
    if layout == "long_spans":
        lengths = before + [6 * block + 11] + after
        start = boundary - sum(before) - (3 * block + 5)
    else:
        lengths = before + [min(wave, 37)] + after
        start = boundary - sum(before) - 1
    offsets = offsets_from(start, [lengths], total)
    assert offsets[len(before)] < boundary < offsets[len(before) + 1] and offsets[-1] < total - 5
    nseg = offsets.size - 1
    need(total * es)
    data = Guarded(total * es, block * es, shift=es if layout == "wave_starts_below" else 0)
    dv = data.view(torch.int32)
    fill(dv, hash32)
    off = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    scan = G.BlellochScan(getattr(G, "DataType_" + dt))
    scan.prepare_batch(total, nseg)
    on_stream(lambda s: scan.run_batch_offsets_ptr(data.ptr, total, off.data_ptr(), nseg, stream=s))
    assert scan.read_batch() == count_classes(lambda c: G.plan_scan_batch(c, es)[0], lengths)
    check_scanned_region(dv, comps, offsets, hash32)
    for lo, hi in list(chunks(int(offsets[0]) * comps)) + [(int(offsets[-1]) * comps, total * comps)]:
        assert bool((u32(dv[lo:hi]) == hash32(iota(lo, hi))).all()), "data outside the segments changed in [%d, %d)" % (lo, hi)
    assert data.intact()
    del scan, data, dv, off
    release()


def test_batched_scan_one_segment_at_the_limit(G):
    """total = 2^32 - 1 uint32 (16 GiB, in place): one segment [0, total) among empty ones, against a running cumsum per chunk."""
    import torch

    total = (1 << 32) - 1
    offsets = np.array([0, 0, 0, total, total, total], dtype=np.int64)
    need(4 * total)
    data = Guarded(4 * total, 1 << 16)
    dv = data.view(torch.int32)
    fill(dv, hash32)
    off = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    scan = G.BlellochScan(G.DataType_Uint)
    scan.prepare_batch(total, 5)
    on_stream(lambda s: scan.run_batch_offsets_ptr(data.ptr, total, off.data_ptr(), 5, stream=s))
    assert scan.read_batch() == {"wave": 0, "block": 0, "long": 1}
    carry = 0
    for lo, hi in chunks(total):
        x = hash32(iota(lo, hi))
        incl = torch.cumsum(x, 0, dtype=torch.int64)
        same = u32(dv[lo:hi]) == ((incl - x + carry) & M32)
        if not bool(same.all()):
            raise AssertionError("element %d" % (lo + int(torch.nonzero(~same)[0])))
        carry = (carry + int(incl[-1])) & M32
        del x, incl, same
    assert data.intact()
    del scan, data, dv, off
    release()


# ------------------------------------------------------------------------------------------------------------ batched sort


@pytest.mark.parametrize("key_type,boundary,room", [("uint32", 1 << 31, 1 << 20), ("uint64", 1 << 29, 1 << 18)])
def test_batched_sort_around_2_31_elements_and_4_gib(G, key_type, boundary, room):
    """uint32 pairs around element 2^31 (total 2^31 + 2^20 + 5: 8 GiB of keys, 8 GiB of values) and uint64 keys with values around
    byte 2^32 of the keys (total 2^29 + 2^18 + 5): about 2000 segments of the three classes on both sides of the boundary, a
    streaming-class segment across it, another one up to nine elements from the end.  Every segment against a stable torch sort of
    it; the elements outside the segments, most of the array, are untouched."""
    import torch

    kb = 8 if key_type == "uint64" else 4
    path_of = lambda c: G.plan_batch(c, kb, True)[0]
    wave, block = last_where(lambda c: path_of(c) <= 1), last_where(lambda c: path_of(c) <= 2)
    total = boundary + room + 5
    per_side = 1000 if kb == 4 else 300  # (what fits behind the boundary)
    k = np.arange(per_side)

    def side(seed):
        lens = hash32_host(k + seed) % (wave + wave // 2) * ((k // 5) % 4 != 0)
        lens[k % 50 == 7] = block - hash32_host(k[k % 50 == 7] + seed) % 100
        lens[k % 200 == 11] = block + 1 + hash32_host(k[k % 200 == 11] + seed) % block
        return lens

    before, after = side(100).astype(np.int64), side(200).astype(np.int64)
    start = boundary - int(before.sum()) - block - 5
    offsets = offsets_from(start, [before, 2 * block + 77, after], total - 9)
    offsets = np.concatenate([offsets, [total - 9]])  # (the last segment takes the rest)
    lengths = np.diff(offsets)
    nseg = lengths.size
    assert offsets[per_side] < boundary < offsets[per_side + 1] and path_of(int(lengths[-1])) == 3
    classes = count_classes(path_of, lengths)
    assert min(classes.values()) > 0
    need(total * (kb + 4))
    keys, vals = Guarded(total * kb, block * kb), Guarded(total * 4, block * 4)
    if kb == 4:
        kv, key_of = keys.view(torch.int32), lambda i: hash32(i) & 0xFFF000FF
    else:
        kv, key_of = keys.view(torch.int64), lambda i: hash64(i) & 0x7F000000000000FF
    vv = vals.view(torch.int32)
    fill(kv, key_of)
    fill(vv, lambda i: i)
    off = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    sorter = G.RadixSort()
    sorter.prepare_batch(total, nseg, kb, True)
    on_stream(lambda s: sorter.sort_batch_offsets_ptr(keys.ptr, vals.ptr, total, off.data_ptr(), nseg, key_type, stream=s))
    assert sorter.read_batch() == classes
    b, e = int(offsets[0]), int(offsets[-1])
    i = iota(b, e)
    k0 = key_of(i)
    seg = torch.repeat_interleave(torch.arange(nseg, device="cuda"), torch.from_numpy(lengths).cuda())
    by_key = torch.sort(k0, stable=True)[1]
    order = by_key[torch.sort(seg[by_key], stable=True)[1]]
    got_k = u32(kv[b:e]) if kb == 4 else kv[b:e]
    same = (got_k == k0[order]) & (u32(vv[b:e]) == (i[order] & M32))
    if not bool(same.all()):
        r = int(torch.nonzero(~same)[0])
        s = int(seg[r])
        raise AssertionError("element %d, segment %d = [%d, %d)" % (b + r, s, int(offsets[s]), int(offsets[s + 1])))
    del i, k0, seg, by_key, order, got_k, same
    for lo, hi in list(chunks(b)) + [(e, total)]:
        j = iota(lo, hi)
        assert bool(((u32(kv[lo:hi]) if kb == 4 else kv[lo:hi]) == key_of(j)).all()), "keys outside the segments changed in [%d, %d)" % (lo, hi)
        assert bool((u32(vv[lo:hi]) == (j & M32)).all()), "values outside the segments changed in [%d, %d)" % (lo, hi)
        del j
    assert keys.intact() and vals.intact()
    del sorter, keys, vals, kv, vv, off
    release()
