"""What every operator refuses, and a few edge cases it accepts, held against a record: tests/golden/refusals.json holds the status,
the whole message (glu_last_error) and, where the unit has one, what *_last reports afterwards, for every call of CASES below.  The
record is never written from the code under test: record() wrote every case up to scan_batch.* from the library of the commit BEFORE the
argument checks moved into csrc/glu_args.hpp, and the radix_sort.* and dist.* cases (the sort's own entry points and the sharded sort's)
from the library of the commit before THOSE entry points moved onto that layer.  A check that changes its place in the order, its text or
its status shows here.  Not in the record: what glu_dist_create and glu_dist_unique_id refuse (both ask for RCCL first), and with them a
NULL out-parameter beside a live glu_dist handle.

CASES is one table.  Plan entry points, and the few handle checks that come before the library asks for its device, need no device and
run unmarked; everything else that takes an object is marked gpu.  The arrays
are two 4 KiB device allocations A and B (zeroed); no message holds an address, no refused call launches a kernel.  The cases run in
the table's order on one object per unit, so *_last after a refused call is what the accepted call before it left."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refusals.json")
U32, I32, F32, U64, I64, F64, BAD_KEY = 0, 1, 2, 3, 4, 5, 9
UINT, DOUBLE, BYTE = 3, 1, 12  # data / stencil types
T32 = 1 << 32
EVEN, EDGES = 0, 1

# the units that have a *_last: (function, number of words)
LAST = {"merge": ("glu_merge_last", 2), "sorted_search": ("glu_sorted_search_last", 3), "histogram": ("glu_histogram_last", 3),
        "expand": ("glu_expand_last", 2)}
CREATE = {"merge": ("glu_merge_create",), "sorted_search": ("glu_sorted_search_create",), "histogram": ("glu_histogram_create",),
          "expand": ("glu_expand_create",), "select": ("glu_select_create",), "key_runs": ("glu_key_runs_create",),
          "scan": ("glu_scan_create", UINT), "reduce": ("glu_reduce_create", UINT, 0), "scan_d": ("glu_scan_create", DOUBLE),
          "sort": ("glu_radix_sort_create",), "radix_sort": ("glu_radix_sort_create",)}
DESTROY = {"scan_d": "glu_scan_destroy", "sort": "glu_radix_sort_destroy"}


class Ctx:
    """The objects and the two arrays of a run of the table; made on first use, so that the plan cases touch no device."""

    def __init__(self, G):
        self.G, self.L = G, G.lib()
        self._h, self._bufs = {}, None
        self.lo, self.hi = ctypes.c_uint32(0), ctypes.c_uint32(64)
        self.flo, self.fhi = ctypes.c_float(1.0), ctypes.c_float(0.0)
        self.tmp = ctypes.c_void_p()
        self.word, self.size = ctypes.c_uint32(), ctypes.c_size_t()
        # host arrays of the sharded sort's plan calls: two ranks' histograms, owners (good, one too large, one negative), outputs
        self.hist = (ctypes.c_uint32 * 512)(*[1] * 512)
        self.owner, self.owner_high, self.owner_negative = [(ctypes.c_int * 256)(*([0] * 128 + [1] * 128)) for _ in range(3)]
        self.owner_high[3], self.owner_negative[255] = 2, -1
        self.send, self.recv, self.cut = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)(), (ctypes.c_int * 18)()

    def h(self, unit):
        if unit not in self._h:
            out = ctypes.c_void_p()
            spec = CREATE[unit]
            self.G.check(getattr(self.L, spec[0])(*spec[1:], ctypes.byref(out)))
            self._h[unit] = out
        return self._h[unit]

    def _arrays(self):
        if self._bufs is None:
            self._bufs = [self.G.ShaderStorageBuffer(size=4096), self.G.ShaderStorageBuffer(size=4096)]
            for b in self._bufs:
                b.clear(0)
        return self._bufs

    A = property(lambda self: self._arrays()[0].device_ptr())
    B = property(lambda self: self._arrays()[1].device_ptr())
    bufA = property(lambda self: self._arrays()[0].handle())

    def ref(self, x):
        return ctypes.byref(x)

    def close(self):
        for unit, handle in self._h.items():
            getattr(self.L, DESTROY.get(unit, "glu_%s_destroy" % unit))(handle)
        for b in self._bufs or []:
            b.destroy()
        self._h, self._bufs = {}, None


def _merge(c, h="merge", a=0, av=1024, na=8, b=256, bv=1280, nb=8, ok=2048, ov=3072, kt=U32, vals=True):
    """glu_merge_run_ptr on A: the six arrays at byte offsets into A (None: NULL)"""
    p = lambda off: None if off is None else c.A + off
    if not vals:
        av = bv = ov = None
    return (c.h(h) if h else None, p(a), p(av), na, p(b), p(bv), nb, p(ok), p(ov), kt, None)


def _search(c, h="sorted_search", hay=0, nh=16, needles=1024, nn=8, kt=U32, lower=2048, upper=3072, reuse=0):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(hay), nh, p(needles), nn, kt, p(lower), p(upper), reuse, None)


def _select(c, h="select", stencil=0, st=UINT, op=1, count=16, items=1024, ib=4, out_items=2048, out_indices=3072, max_out=16, num=4000):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(stencil), st, op, None, count, p(items), ib, p(out_items), p(out_indices), max_out, p(num), None)


def _runs(c, h="key_runs", keys=0, count=16, bits=32, begin=0, end=32, unique=1024, offsets=2048, max_runs=16, num=4000):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(keys), count, bits, begin, end, p(unique), p(offsets), max_runs, p(num), None)


def _even(c, h="histogram", samples=0, count=16, kt=U32, lo="lo", hi="hi", bins=16, out=2048, acc=0):
    p = lambda off: None if off is None else c.A + off
    r = lambda name: None if name is None else c.ref(getattr(c, name))
    return (c.h(h) if h else None, p(samples), count, kt, r(lo), r(hi), bins, p(out), acc, None)


def _edges(c, h="histogram", samples=0, count=16, kt=U32, edges=1024, bins=16, out=2048, acc=0):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(samples), count, kt, p(edges), bins, p(out), acc, None)


def _expand(c, h="expand", offsets=0, nseg=4, total=16, items=512, ib=4, out_items=1024, segs=2048, ranks=3072):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(offsets), nseg, total, p(items), ib, p(out_items), p(segs), p(ranks), None)


def _sort_eq(c, h="sort", keys=0, vals=2048, count=4, parts=2, kt=U32):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(keys), p(vals), count, parts, kt, None)


def _sort_off(c, h="sort", keys=0, vals=2048, total=8, offsets=0, nseg=2, kt=U32):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(keys), p(vals), total, None if offsets is None else c.B + offsets, nseg, kt, None)


def _red_eq(c, h="reduce", data=0, out=2048, count=4, parts=2):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(data), p(out), count, parts, None)


def _red_off(c, h="reduce", data=0, out=2048, total=8, offsets=0, nseg=2):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(data), p(out), total, None if offsets is None else c.B + offsets, nseg, None)


def _scan_off(c, h="scan", data=0, total=8, offsets=0, nseg=2):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(data), total, None if offsets is None else c.B + offsets, nseg, None)


def _sort_ptr(c, h="radix_sort", keys=0, vals=2048, count=16, tail=(0,)):
    """a *_ptr sort on A: handle, keys, vals (False: the entry point takes none), count, `tail` (steps / key type / bits), stream"""
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(keys)) + (() if vals is False else (p(vals),)) + (count,) + tuple(tail) + (None,)


def _sort_buf(c, h="radix_sort", keys="bufA", vals="bufA", count=16):
    """a sort of buffer handles (a name: that buffer of c; a number: that handle)"""
    b = lambda x: getattr(c, x) if isinstance(x, str) else x
    return (c.h(h) if h else None, b(keys)) + (() if vals is False else (b(vals),)) + (count, 0)


def _sort_part(c, h="radix_sort", sk=0, sv=1024, dk=2048, dv=3072, count=16, shift=24, bits=8):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(sk), p(sv), p(dk), p(dv), count, shift, bits, None, None)


def _pieces(begin, length, seg):
    """the three piece arrays of a segmented sort (None: NULL)"""
    arr = lambda t, v: None if v is None else (t * max(len(v), 1))(*v)
    return arr(ctypes.c_uint64, begin), arr(ctypes.c_uint64, length), arr(ctypes.c_uint32, seg)


def _sort_seg(c, h="radix_sort", ik=0, iv=1024, ok=2048, ov=3072, count=8, begin=(0, 4), length=(4, 4), seg=(0, 1), n=2, nseg=2, bits=32):
    p = lambda off: None if off is None else c.A + off
    return (c.h(h) if h else None, p(ik), p(iv), p(ok), p(ov), count) + _pieces(begin, length, seg) + (n, nseg, bits, None)


def _plan_seg(c, begin=(0, 4), length=(4, 4), seg=(0, 1), n=2, nseg=2, nwg=4, cap=64, num=True):
    """glu_radix_sort_plan_segments with room for `cap` sub-blocks (the outputs of a refused call are never written)"""
    room = lambda t, k: (t * (min(k, 64) + 1))()
    return _pieces(begin, length, seg) + (n, nseg, nwg, room(ctypes.c_uint32, 2 * cap), cap, room(ctypes.c_uint32, nwg), room(ctypes.c_uint32, nseg),
                                          room(ctypes.c_uint64, nseg), c.ref(c.size) if num else None)


def case(name, fn, args, gpu=True):
    return {"name": name, "fn": fn, "args": args, "gpu": gpu}


def plan(name, fn, *args):
    """a plan entry point with every out-parameter NULL; the outs are counted from the argtypes"""
    return case(name, fn, lambda c: args, gpu=False)


def M(name, **kw):
    return case("merge.run." + name, "glu_merge_run_ptr", lambda c: _merge(c, **kw))


def S(name, **kw):
    return case("sorted_search.run." + name, "glu_sorted_search_run_ptr", lambda c: _search(c, **kw))


def SE(name, **kw):
    return case("select.run." + name, "glu_select_run_ptr", lambda c: _select(c, **kw))


def KR(name, **kw):
    return case("key_runs.run." + name, "glu_key_runs_run_ptr", lambda c: _runs(c, **kw))


def HE(name, **kw):
    return case("histogram.even." + name, "glu_histogram_run_even_ptr", lambda c: _even(c, **kw))


def HD(name, **kw):
    return case("histogram.edges." + name, "glu_histogram_run_edges_ptr", lambda c: _edges(c, **kw))


def EX(name, **kw):
    return case("expand.run." + name, "glu_expand_run_ptr", lambda c: _expand(c, **kw))


def RS(entry, name, build=_sort_ptr, **kw):
    return case("radix_sort.%s.%s" % (entry, name), "glu_radix_sort_" + entry, lambda c: build(c, **kw))


def host(name, fn, args):
    """a call that needs no device and has no out-parameter to make: `args` is the whole argument list"""
    return case(name, fn, args, gpu=False)


CASES = [
    # ---- merge
    plan("merge.plan.ok", "glu_merge_plan", 100, 50, U32, 1),
    plan("merge.plan.key_type", "glu_merge_plan", 8, 8, BAD_KEY, 1),
    plan("merge.plan.key_type_negative", "glu_merge_plan", 8, 8, -1, 1),
    plan("merge.plan.key_type+total", "glu_merge_plan", T32, 8, BAD_KEY, 1),
    plan("merge.plan.a_count", "glu_merge_plan", T32, 0, U32, 1),
    plan("merge.plan.sum", "glu_merge_plan", 1 << 31, 1 << 31, U64, 0),
    case("merge.create.null", "glu_merge_create", lambda c: (None,)),
    case("merge.destroy.null", "glu_merge_destroy", lambda c: (None,)),
    case("merge.prepare.null", "glu_merge_prepare", lambda c: (None, 64, U32)),
    case("merge.prepare.null+key_type", "glu_merge_prepare", lambda c: (None, 64, BAD_KEY)),
    case("merge.prepare.key_type", "glu_merge_prepare", lambda c: (c.h("merge"), 64, BAD_KEY)),
    case("merge.prepare.key_type+total", "glu_merge_prepare", lambda c: (c.h("merge"), T32, BAD_KEY)),
    case("merge.prepare.total", "glu_merge_prepare", lambda c: (c.h("merge"), T32, U32)),
    case("merge.last.null", "glu_merge_last", lambda c: (None, None, None)),
    M("null", h=None),
    M("null+key_type", h=None, kt=BAD_KEY),
    M("key_type", kt=6),
    M("key_type+total", kt=BAD_KEY, na=T32),
    M("total", na=1 << 31, nb=1 << 31),
    M("a_keys_null", a=None),
    M("b_keys_null", b=None),
    M("out_keys_null", ok=None),
    M("a_vals_missing", av=None),
    M("b_vals_missing", bv=None),
    M("out_vals_missing", ov=None),
    M("a_keys_align", a=2),
    M("b_keys_align", b=260, kt=I64),
    M("out_keys_align", ok=2052, kt=F64),
    M("a_vals_align", av=1025),
    M("b_vals_align", bv=1282),
    M("out_vals_align", ov=3075),
    M("a_keys_align+b_keys_align", a=2, b=258),
    M("out_keys_align+overlap", ok=2, a=0),
    M("out_keys_overlaps_a_keys", ok=0),
    M("out_keys_overlaps_a_keys_tail", ok=28),
    M("out_keys_adjacent_a_keys", ok=32, na=8, b=256, nb=8),
    M("out_keys_overlaps_b_keys", ok=256 - 4 * 15),
    M("out_keys_overlaps_a_vals", ok=1024),
    M("out_keys_overlaps_b_vals", ok=1280),
    M("out_vals_overlaps_a_keys", ov=0),
    M("out_vals_overlaps_b_vals", ov=1280 + 28),
    M("out_vals_overlaps_out_keys", ov=2048 + 4 * 15),
    M("two_pairs_out_keys_b_keys+out_vals_a_keys", ok=256, ov=0),
    M("two_pairs_out_keys_b_keys+out_keys_a_vals", ok=1024, av=1024, b=1028, nb=1),
    M("two_pairs_out_vals_out_keys+out_vals_b_vals", ov=2048, bv=2048),
    M("ok_keys_only", vals=False),
    M("ok_a_empty_null", a=None, av=None, na=0),
    M("ok_b_empty_null", b=None, bv=None, nb=0),
    M("ok_both_empty_null", a=None, av=None, na=0, b=None, bv=None, nb=0, ok=None, ov=None),
    M("total_after_ok", na=T32 - 1, nb=1),
    M("a_empty_misaligned_not_looked_at", a=2, na=0),
    # ---- sorted search
    plan("sorted_search.plan.ok", "glu_sorted_search_plan", 1 << 20, 1 << 16, U32, 0),
    plan("sorted_search.plan.key_type", "glu_sorted_search_plan", 16, 16, BAD_KEY, 0),
    plan("sorted_search.plan.key_type+hay_count", "glu_sorted_search_plan", T32, 16, BAD_KEY, 0),
    plan("sorted_search.plan.hay_count", "glu_sorted_search_plan", T32, 16, U32, 0),
    plan("sorted_search.plan.hay_count+needle_count", "glu_sorted_search_plan", T32, T32, U32, 0),
    plan("sorted_search.plan.needle_count", "glu_sorted_search_plan", 16, T32, U64, 0),
    plan("sorted_search.plan.top_entries_low", "glu_sorted_search_plan", 16, 16, U32, 16),
    plan("sorted_search.plan.top_entries_high", "glu_sorted_search_plan", 16, 16, U64, 8192),
    case("sorted_search.create.null", "glu_sorted_search_create", lambda c: (None,)),
    case("sorted_search.destroy.null", "glu_sorted_search_destroy", lambda c: (None,)),
    case("sorted_search.prepare.null", "glu_sorted_search_prepare", lambda c: (None, 64, BAD_KEY)),
    case("sorted_search.prepare.key_type", "glu_sorted_search_prepare", lambda c: (c.h("sorted_search"), T32, BAD_KEY)),
    case("sorted_search.prepare.hay_count", "glu_sorted_search_prepare", lambda c: (c.h("sorted_search"), T32, U32)),
    case("sorted_search.set_option.null", "glu_sorted_search_set_option", lambda c: (None, None, 0)),
    case("sorted_search.set_option.name_null", "glu_sorted_search_set_option", lambda c: (c.h("sorted_search"), None, 0)),
    case("sorted_search.set_option.path", "glu_sorted_search_set_option", lambda c: (c.h("sorted_search"), b"PATH", 3)),
    case("sorted_search.set_option.top_entries", "glu_sorted_search_set_option", lambda c: (c.h("sorted_search"), b"TOP_ENTRIES", 8)),
    case("sorted_search.set_option.unknown", "glu_sorted_search_set_option", lambda c: (c.h("sorted_search"), b"FANOUT", 8)),
    case("sorted_search.last.null", "glu_sorted_search_last", lambda c: (None, None, None, None)),
    case("sorted_search.index.null", "glu_sorted_search_index_ptr", lambda c: (None, c.A, 16, BAD_KEY, None)),
    case("sorted_search.index.key_type", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), c.A, T32, BAD_KEY, None)),
    case("sorted_search.index.hay_count", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), None, T32, U32, None)),
    case("sorted_search.index.hay_null", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), None, 16, U32, None)),
    case("sorted_search.index.hay_align", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), c.A + 4, 16, U64, None)),
    S("null+key_type", h=None, kt=BAD_KEY),
    S("key_type+hay_count", kt=BAD_KEY, nh=T32),
    S("hay_count+needle_count", nh=T32, nn=T32),
    S("needle_count", nn=T32),
    S("hay_null", hay=None),
    S("hay_align", hay=2),
    S("hay_align+needles_null", hay=2, needles=None),
    S("needles_null", needles=None),
    S("needles_null+both_out_null", needles=None, lower=None, upper=None),
    S("both_out_null", lower=None, upper=None),
    S("both_out_null+needles_align", lower=None, upper=None, needles=1026),
    S("needles_align", needles=1028, kt=I64),
    S("out_lower_align", lower=2050),
    S("out_upper_align", upper=3073),
    S("out_lower_align+overlap", lower=2, upper=0),
    S("out_lower_overlaps_hay", lower=60),
    S("out_lower_adjacent_hay", lower=64),
    S("out_lower_overlaps_needles", lower=1024 + 28),
    S("out_upper_overlaps_hay", upper=0),
    S("out_upper_overlaps_needles", upper=1024),
    S("out_upper_overlaps_out_lower", upper=2048 + 28),
    S("two_pairs_out_lower_needles+out_upper_hay", lower=1024, upper=0),
    S("two_pairs_out_upper_needles+out_upper_out_lower", lower=2048, upper=2048, needles=2048 + 16),
    S("reuse_no_index", reuse=1),
    S("ok_direct"),
    S("ok_lower_only", upper=None),
    S("ok_no_needles_null", needles=None, nn=0),
    S("ok_no_hay_null", hay=None, nh=0),
    case("sorted_search.index.ok", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), c.A, 16, U32, None)),
    S("reuse_other_hay", reuse=1, nh=15),
    S("ok_reuse", reuse=1),
    S("key_type_after_ok", kt=-1),
    case("sorted_search.set_option.ok_top_entries_16", "glu_sorted_search_set_option", lambda c: (c.h("sorted_search"), b"TOP_ENTRIES", 16)),
    S("top_entries_for_key_width"),
    S("hay_align+top_entries", hay=2),
    case("sorted_search.prepare.top_entries", "glu_sorted_search_prepare", lambda c: (c.h("sorted_search"), 64, U32)),
    case("sorted_search.index.top_entries", "glu_sorted_search_index_ptr", lambda c: (c.h("sorted_search"), c.A, 16, U32, None)),
    # ---- select
    plan("select.plan.ok", "glu_select_plan", 100000, UINT),
    plan("select.plan.stencil_type", "glu_select_plan", 16, 4),
    plan("select.plan.stencil_type+count", "glu_select_plan", T32, 4),
    plan("select.plan.count", "glu_select_plan", T32, BYTE),
    case("select.create.null", "glu_select_create", lambda c: (None,)),
    case("select.destroy.null", "glu_select_destroy", lambda c: (None,)),
    case("select.prepare.null", "glu_select_prepare", lambda c: (None, 16, 4)),
    case("select.prepare.stencil_type", "glu_select_prepare", lambda c: (c.h("select"), T32, 4)),
    case("select.prepare.count", "glu_select_prepare", lambda c: (c.h("select"), T32, UINT)),
    SE("null+stencil_type", h=None, st=4),
    SE("stencil_type+op", st=4, op=6),
    SE("op+count", op=-1, count=T32),
    SE("count+max_out", count=T32, max_out=T32),
    SE("max_out", max_out=T32),
    SE("stencil_null", stencil=None),
    SE("stencil_null+num_null", stencil=None, num=None),
    SE("num_null", num=None),
    SE("items_without_out_items", out_items=None),
    SE("out_items_without_items", items=None),
    SE("item_bytes", ib=12),
    SE("item_bytes+items_align", ib=12, items=1026),
    SE("item_bytes+stencil_align", ib=3, stencil=2),
    SE("stencil_align", stencil=4, st=DOUBLE),
    SE("stencil_align+items_align", stencil=2, items=1028, ib=8),
    SE("items_align_8", items=1028, ib=8),
    SE("items_align_32", items=1032, ib=32, count=4, max_out=4),
    SE("out_items_align_16", out_items=2056, ib=16, count=4, max_out=4),
    SE("out_indices_align", out_indices=3074),
    SE("num_align", num=4002),
    SE("num_align+overlap", num=2, stencil=0),
    SE("out_items_overlaps_stencil", out_items=32),
    SE("out_items_adjacent_stencil", out_items=64),
    SE("out_items_overlaps_items", out_items=1024 + 60),
    SE("out_indices_overlaps_stencil", out_indices=0),
    SE("out_indices_overlaps_items", out_indices=1024),
    SE("num_overlaps_stencil", num=60),
    SE("num_overlaps_items", num=1024),
    SE("two_pairs_out_items_items+out_indices_stencil", out_items=1024, out_indices=0),
    SE("ok_out_items_is_out_indices", out_items=2048, out_indices=2048),
    SE("ok_max_out_bounds_the_overlap", out_items=60, max_out=0),
    SE("ok_no_items_item_bytes_ignored", items=None, out_items=None, ib=12),
    SE("ok_count_0_stencil_null", stencil=None, count=0),
    # ---- key runs
    plan("key_runs.plan.ok", "glu_key_runs_plan", 100000, 64),
    plan("key_runs.plan.key_bits", "glu_key_runs_plan", T32, 16),
    plan("key_runs.plan.count", "glu_key_runs_plan", T32, 32),
    case("key_runs.create.null", "glu_key_runs_create", lambda c: (None,)),
    case("key_runs.destroy.null", "glu_key_runs_destroy", lambda c: (None,)),
    case("key_runs.prepare.null", "glu_key_runs_prepare", lambda c: (None, 16, 16)),
    case("key_runs.prepare.key_bits", "glu_key_runs_prepare", lambda c: (c.h("key_runs"), T32, 16)),
    case("key_runs.prepare.count", "glu_key_runs_prepare", lambda c: (c.h("key_runs"), T32, 64)),
    KR("null+key_bits", h=None, bits=16),
    KR("key_bits+count", bits=48, count=T32),
    KR("count+max_runs", count=T32, max_runs=T32),
    KR("max_runs+bit_range", max_runs=T32, begin=8, end=4),
    KR("bit_range_order", begin=8, end=4),
    KR("bit_range_end", end=33),
    KR("bit_range+keys_null", end=33, keys=None),
    KR("keys_null", keys=None),
    KR("offsets_null", offsets=None),
    KR("num_runs_null", num=None),
    KR("num_runs_null+keys_align", num=None, keys=2),
    KR("keys_align", keys=4, bits=64, end=64),
    KR("unique_keys_align", unique=1026),
    KR("offsets_align", offsets=2049),
    KR("num_runs_align", num=4002),
    KR("keys_align+unique_keys_align", keys=2, unique=1026),
    KR("num_runs_align+overlap", num=2),
    KR("offsets_overlaps_keys", offsets=60),
    KR("offsets_overlaps_keys_by_its_last_entry", keys=2048 + 64, offsets=2048),
    KR("offsets_adjacent_keys", keys=2048 + 68, offsets=2048),
    KR("unique_keys_overlaps_keys", unique=60),
    KR("unique_keys_adjacent_keys", unique=64),
    KR("num_runs_overlaps_keys", num=0),
    KR("two_pairs_offsets_keys+unique_keys_keys", offsets=0, unique=0),
    KR("two_pairs_unique_keys_keys+num_runs_keys", unique=32, num=32),
    KR("ok_unique_keys_null", unique=None),
    KR("ok_count_0_keys_null", keys=None, count=0),
    KR("ok_unique_keys_is_offsets", unique=2048),
    # ---- histogram
    plan("histogram.plan.ok", "glu_histogram_plan", 100000, 100, U32, EVEN),
    plan("histogram.plan.key_type+mode", "glu_histogram_plan", 16, 16, BAD_KEY, 2),
    plan("histogram.plan.mode+count", "glu_histogram_plan", T32, 16, U32, 2),
    plan("histogram.plan.count+bins", "glu_histogram_plan", T32, 0, U32, EVEN),
    plan("histogram.plan.bins_0", "glu_histogram_plan", 16, 0, U32, EVEN),
    plan("histogram.plan.bins_even_most", "glu_histogram_plan", 16, T32, F32, EVEN),
    plan("histogram.plan.bins_edges_most", "glu_histogram_plan", 16, 8193, U64, EDGES),
    plan("histogram.plan.bins+wide_even", "glu_histogram_plan", 16, 0, U64, EVEN),
    plan("histogram.plan.wide_even_u64", "glu_histogram_plan", 16, 16, U64, EVEN),
    plan("histogram.plan.wide_even_i64", "glu_histogram_plan", 16, 16, I64, EVEN),
    case("histogram.create.null", "glu_histogram_create", lambda c: (None,)),
    case("histogram.destroy.null", "glu_histogram_destroy", lambda c: (None,)),
    case("histogram.prepare.null", "glu_histogram_prepare", lambda c: (None, T32, 16)),
    case("histogram.prepare.count", "glu_histogram_prepare", lambda c: (c.h("histogram"), T32, 16)),
    case("histogram.prepare.bins", "glu_histogram_prepare", lambda c: (c.h("histogram"), 16, 0)),
    case("histogram.last.null", "glu_histogram_last", lambda c: (None, None, None, None)),
    HE("null+key_type", h=None, kt=BAD_KEY),
    HE("key_type+count", kt=BAD_KEY, count=T32),
    HE("count+lo_null", count=T32, lo=None),
    HE("wide+lo_null", kt=I64, lo=None),
    HE("lo_null+hi_null", lo=None, hi=None),
    HE("hi_null+samples_null", hi=None, samples=None),
    HE("samples_null+out_null", samples=None, out=None),
    HE("out_null+samples_align", out=None, samples=2),
    HE("samples_align+out_align", samples=4, kt=F64, lo="flo", hi="fhi", out=2050),
    HE("samples_align", samples=2),
    HE("out_align+overlap", out=2),
    HE("out_overlaps_samples", out=60),
    HE("out_adjacent_samples", out=64),
    HE("overlap+uneven_int_bins", out=0, bins=5),
    HE("uneven_int_bins", bins=5),
    HE("float_bounds", kt=F32, lo="flo", hi="fhi"),
    HE("ok"),
    HE("ok_count_0", samples=None, count=0),
    HE("ok_count_0_misaligned_not_looked_at", samples=2, count=0),
    HE("ok_count_0_accumulate", samples=None, count=0, acc=1),
    HE("key_type_after_ok", kt=-1),
    HD("null+key_type", h=None, kt=BAD_KEY),
    HD("key_type+bins", kt=BAD_KEY, bins=8193),
    HD("bins_most", bins=8193),
    HD("bins_0+samples_null", bins=0, samples=None),
    HD("samples_null", samples=None),
    HD("out_null+edges_null", out=None, edges=None),
    HD("edges_null+samples_align", edges=None, samples=2),
    HD("samples_align+edges_align", samples=4, edges=1028, kt=U64),
    HD("out_align+edges_align", out=2049, edges=1026),
    HD("edges_align", edges=1028, kt=I64),
    HD("edges_align+overlap", edges=1026, out=0),
    HD("out_overlaps_samples+out_overlaps_edges", samples=0, edges=32, out=0, count=8, bins=8),
    HD("out_overlaps_edges", out=1024 + 32),
    HD("out_overlaps_edges_by_the_last_edge", out=1024 + 64, bins=16),
    HD("out_adjacent_edges", out=1024 + 68),
    HD("ok"),
    HD("ok_wide", kt=F64),
    HD("ok_count_0", samples=None, count=0),
    HD("ok_count_0_accumulate", samples=None, count=0, acc=1),
    # ---- expand
    plan("expand.plan.ok", "glu_expand_plan", 100000, 3000),
    plan("expand.plan.num_segments+total", "glu_expand_plan", T32, (1 << 24) + 1),
    plan("expand.plan.total", "glu_expand_plan", T32, 4),
    plan("expand.plan.sum", "glu_expand_plan", T32 - 4, 4),
    case("expand.create.null", "glu_expand_create", lambda c: (None,)),
    case("expand.destroy.null", "glu_expand_destroy", lambda c: (None,)),
    case("expand.prepare.null", "glu_expand_prepare", lambda c: (None, T32, 4)),
    case("expand.prepare.total", "glu_expand_prepare", lambda c: (c.h("expand"), T32, 4)),
    case("expand.last.null", "glu_expand_last", lambda c: (None, None, None)),
    EX("ok"),
    EX("null+sizes", h=None, total=T32),
    EX("sizes+offsets_null", total=T32, offsets=None),
    EX("offsets_null+items_without_out_items", offsets=None, out_items=None),
    EX("items_without_out_items+item_bytes", out_items=None, ib=12),
    EX("out_items_without_items", items=None),
    EX("item_bytes", ib=12),
    EX("item_bytes+items_align", ib=12, items=514),
    EX("item_bytes+offsets_align", ib=0, offsets=2),
    EX("offsets_align+out_segments_align", offsets=2, segs=2049),
    EX("out_segments_align+out_ranks_align", segs=2050, ranks=3073),
    EX("out_ranks_align+items_align", ranks=3074, items=516, ib=8),
    EX("items_align_4", items=514),
    EX("items_align_8+out_items_align", items=516, ib=8, out_items=1028),
    EX("items_align_16", items=520, ib=16, total=8),
    EX("items_align_32", items=520, ib=32, total=8),
    EX("out_items_align_8", out_items=1028, ib=8),
    EX("out_items_align_32", out_items=1032, ib=32, total=8),
    EX("out_items_align+overlap", out_items=2, ib=8),
    EX("out_segments_overlaps_out_ranks", ranks=2048 + 60),
    EX("out_segments_adjacent_out_ranks", ranks=2048 + 64),
    EX("out_segments_overlaps_out_items", out_items=2048),
    EX("out_segments_overlaps_offsets", segs=16),
    EX("out_segments_adjacent_offsets", segs=20),
    EX("out_segments_overlaps_items", segs=512 + 12),
    EX("out_ranks_overlaps_out_items", ranks=1024 + 60),
    EX("out_ranks_overlaps_offsets", ranks=0),
    EX("out_ranks_overlaps_items", ranks=512),
    EX("out_items_overlaps_offsets", out_items=16),
    EX("out_items_overlaps_items", out_items=512),
    EX("two_pairs_out_segments_items+out_ranks_out_items", segs=512, ranks=1024),
    EX("two_pairs_out_segments_offsets+out_segments_out_ranks", segs=0, ranks=0),
    EX("two_pairs_out_ranks_offsets+out_items_items", ranks=0, out_items=512),
    EX("ok_total_0_nothing_looked_at", total=0, offsets=None, items=514, ib=12),
    EX("ok_no_segments", nseg=0, offsets=None),
    EX("ok_no_outputs", items=None, out_items=None, segs=None, ranks=None),
    EX("no_outputs_offsets_align", items=None, out_items=None, segs=None, ranks=None, offsets=2),
    EX("ok_segments_only", items=None, out_items=None, ranks=None),
    EX("sizes_after_ok", nseg=(1 << 24) + 1),
    # ---- scan and reduce
    case("scan.create.null+data_type", "glu_scan_create", lambda c: (99, None)),
    case("scan.create.data_type", "glu_scan_create", lambda c: (12, c.ref(c.tmp))),
    case("scan.create.data_type_negative", "glu_scan_create", lambda c: (-1, c.ref(c.tmp))),
    case("scan.destroy.null", "glu_scan_destroy", lambda c: (None,)),
    case("scan.prepare.null", "glu_scan_prepare", lambda c: (None, 16, 1)),
    case("scan.prepare.ok_count_0", "glu_scan_prepare", lambda c: (c.h("scan"), 0, 1)),
    case("scan.run_ptr.null+data_null", "glu_scan_run_ptr", lambda c: (None, None, 0, 0, None)),
    case("scan.run_ptr.data_null+count", "glu_scan_run_ptr", lambda c: (c.h("scan"), None, 0, 0, None)),
    case("scan.run_ptr.count+partitions", "glu_scan_run_ptr", lambda c: (c.h("scan"), c.A, 0, 0, None)),
    case("scan.run_ptr.partitions+align", "glu_scan_run_ptr", lambda c: (c.h("scan"), c.A + 2, 16, 0, None)),
    case("scan.run_ptr.align", "glu_scan_run_ptr", lambda c: (c.h("scan"), c.A + 2, 16, 1, None)),
    case("scan.run_ptr.align_double", "glu_scan_run_ptr", lambda c: (c.h("scan_d"), c.A + 4, 16, 1, None)),
    case("scan.run_ptr.ok", "glu_scan_run_ptr", lambda c: (c.h("scan"), c.A + 4, 16, 1, None)),
    case("scan.run.null", "glu_scan_run", lambda c: (None, 0, 0, 0)),
    case("scan.run.buffer", "glu_scan_run", lambda c: (c.h("scan"), 0, 0, 0)),
    case("scan.run.count", "glu_scan_run", lambda c: (c.h("scan"), c.bufA, 0, 0)),
    case("scan.run.power_of_2", "glu_scan_run", lambda c: (c.h("scan"), c.bufA, 12, 0)),
    case("scan.run.partitions", "glu_scan_run", lambda c: (c.h("scan"), c.bufA, 16, 0)),
    case("scan.run.size", "glu_scan_run", lambda c: (c.h("scan"), c.bufA, 1024, 2)),
    case("reduce.create.null+data_type", "glu_reduce_create", lambda c: (99, 99, None)),
    case("reduce.create.data_type+op", "glu_reduce_create", lambda c: (12, 4, c.ref(c.tmp))),
    case("reduce.create.op", "glu_reduce_create", lambda c: (UINT, 4, c.ref(c.tmp))),
    case("reduce.destroy.null", "glu_reduce_destroy", lambda c: (None,)),
    case("reduce.run_ptr.null+data_null", "glu_reduce_run_ptr", lambda c: (None, None, 0, None)),
    case("reduce.run_ptr.data_null+count", "glu_reduce_run_ptr", lambda c: (c.h("reduce"), None, 0, None)),
    case("reduce.run_ptr.count+align", "glu_reduce_run_ptr", lambda c: (c.h("reduce"), c.A + 2, 0, None)),
    case("reduce.run_ptr.align", "glu_reduce_run_ptr", lambda c: (c.h("reduce"), c.A + 2, 16, None)),
    case("reduce.run_ptr.ok", "glu_reduce_run_ptr", lambda c: (c.h("reduce"), c.A + 4, 16, None)),
    case("reduce.run.null", "glu_reduce_run", lambda c: (None, 0, 0)),
    case("reduce.run.buffer", "glu_reduce_run", lambda c: (c.h("reduce"), 0, 0)),
    case("reduce.run.count", "glu_reduce_run", lambda c: (c.h("reduce"), c.bufA, 0)),
    case("reduce.run.size", "glu_reduce_run", lambda c: (c.h("reduce"), c.bufA, 1025)),
    # ---- the batched units
    plan("sort_batch.plan.key_bytes", "glu_radix_sort_plan_batch", 16, 2, 1),
    plan("sort_batch.plan.ok", "glu_radix_sort_plan_batch", 1000, 4, 1),
    case("sort_batch.prepare.null", "glu_radix_sort_prepare_batch", lambda c: (None, 16, 2, 2, 1)),
    case("sort_batch.prepare.key_bytes+total", "glu_radix_sort_prepare_batch", lambda c: (c.h("sort"), T32, 2, 2, 1)),
    case("sort_batch.prepare.total+segments", "glu_radix_sort_prepare_batch", lambda c: (c.h("sort"), T32, (1 << 24) + 1, 4, 1)),
    case("sort_batch.prepare.segments", "glu_radix_sort_prepare_batch", lambda c: (c.h("sort"), 16, (1 << 24) + 1, 4, 1)),
    case("sort_batch.read.null", "glu_radix_sort_read_batch", lambda c: (None, None, None, None)),
    case("sort_batch.run.null+key_type", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, h=None, kt=BAD_KEY)),
    case("sort_batch.run.overflow+key_type", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, count=1 << 40, parts=1 << 40, kt=BAD_KEY)),
    case("sort_batch.run.key_type+total", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, count=1 << 31, parts=2, kt=BAD_KEY)),
    case("sort_batch.run.total+keys_null", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, count=1 << 31, parts=2, keys=None)),
    case("sort_batch.run.keys_null+vals_align", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, keys=None, vals=2049)),
    case("sort_batch.run.keys_align+vals_align", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, keys=4, vals=2049, kt=U64)),
    case("sort_batch.run.keys_align", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, keys=2)),
    case("sort_batch.run.vals_align+segments", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, vals=2050, count=1, parts=(1 << 24) + 1)),
    case("sort_batch.run.segments", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, count=1, parts=(1 << 24) + 1)),
    case("sort_batch.run.ok_no_partitions", "glu_radix_sort_run_batch_ptr", lambda c: _sort_eq(c, parts=0, keys=None, vals=None)),
    case("sort_batch.offsets.null+key_type", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, h=None, kt=BAD_KEY)),
    case("sort_batch.offsets.key_type+total", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, kt=6, total=T32)),
    case("sort_batch.offsets.total", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, total=T32)),
    case("sort_batch.offsets.keys_null", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, keys=None)),
    case("sort_batch.offsets.keys_align", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, keys=4, kt=F64)),
    case("sort_batch.offsets.vals_align+segments", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, vals=2049, nseg=(1 << 24) + 1)),
    case("sort_batch.offsets.segments+offsets_null", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, nseg=(1 << 24) + 1, offsets=None)),
    case("sort_batch.offsets.offsets_null", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, offsets=None)),
    case("sort_batch.offsets.offsets_align", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, offsets=2)),
    case("sort_batch.offsets.ok_no_segments", "glu_radix_sort_run_batch_offsets_ptr", lambda c: _sort_off(c, nseg=0, offsets=None)),
    plan("reduce_batch.plan.elem_bytes", "glu_reduce_plan_batch", 16, 12),
    plan("reduce_batch.plan.ok", "glu_reduce_plan_batch", 1000, 4),
    case("reduce_batch.prepare.null", "glu_reduce_prepare_batch", lambda c: (None, T32, 2)),
    case("reduce_batch.prepare.total+segments", "glu_reduce_prepare_batch", lambda c: (c.h("reduce"), T32, (1 << 24) + 1)),
    case("reduce_batch.prepare.segments", "glu_reduce_prepare_batch", lambda c: (c.h("reduce"), 16, (1 << 24) + 1)),
    case("reduce_batch.read.null", "glu_reduce_read_batch", lambda c: (None, None, None, None)),
    case("reduce_batch.run.null+partitions", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, h=None, parts=1 << 31)),
    case("reduce_batch.run.partitions+overflow", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, count=1 << 40, parts=1 << 31)),
    case("reduce_batch.run.overflow+data_null", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, count=1 << 40, parts=1 << 30, data=None)),
    case("reduce_batch.run.data_null+out_null", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, data=None, out=None)),
    case("reduce_batch.run.out_null+data_align", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, out=None, data=2)),
    case("reduce_batch.run.data_align+out_align", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, data=2, out=2049)),
    case("reduce_batch.run.out_align+overlap", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, out=2)),
    case("reduce_batch.run.address_space", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, count=1 << 40, parts=1 << 22)),
    case("reduce_batch.run.out_overlaps_data", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, out=28)),
    case("reduce_batch.run.out_adjacent_data", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, out=32)),
    case("reduce_batch.run.ok_no_partitions", "glu_reduce_run_batch_ptr", lambda c: _red_eq(c, parts=0, data=None, out=None)),
    case("reduce_batch.offsets.null+total", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, h=None, total=T32)),
    case("reduce_batch.offsets.total+segments", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, total=T32, nseg=(1 << 24) + 1)),
    case("reduce_batch.offsets.segments+data_null", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, nseg=(1 << 24) + 1, data=None)),
    case("reduce_batch.offsets.data_null", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, data=None)),
    case("reduce_batch.offsets.out_overlaps_data+offsets_null", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, out=28, offsets=None)),
    case("reduce_batch.offsets.offsets_null", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, offsets=None)),
    case("reduce_batch.offsets.offsets_align", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, offsets=2)),
    case("reduce_batch.offsets.ok_no_segments", "glu_reduce_run_batch_offsets_ptr", lambda c: _red_off(c, nseg=0, data=None, out=None, offsets=None)),
    plan("scan_batch.plan.elem_bytes", "glu_scan_plan_batch", 16, 12),
    plan("scan_batch.plan.ok", "glu_scan_plan_batch", 1000, 4),
    case("scan_batch.prepare.null", "glu_scan_prepare_batch", lambda c: (None, T32, 2)),
    case("scan_batch.prepare.total+segments", "glu_scan_prepare_batch", lambda c: (c.h("scan"), T32, (1 << 24) + 1)),
    case("scan_batch.prepare.segments", "glu_scan_prepare_batch", lambda c: (c.h("scan"), 16, (1 << 24) + 1)),
    case("scan_batch.read.null", "glu_scan_read_batch", lambda c: (None, None, None, None)),
    case("scan_batch.offsets.null+total", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, h=None, total=T32)),
    case("scan_batch.offsets.total+segments", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, total=T32, nseg=(1 << 24) + 1)),
    case("scan_batch.offsets.segments", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, nseg=(1 << 24) + 1)),
    case("scan_batch.offsets.ok_no_segments_nothing_looked_at", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, nseg=0, data=2, offsets=None)),
    case("scan_batch.offsets.data_null+offsets_null", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, data=None, offsets=None)),
    case("scan_batch.offsets.offsets_null+data_align", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, offsets=None, data=2)),
    case("scan_batch.offsets.offsets_align+data_align", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, offsets=2, data=2)),
    case("scan_batch.offsets.data_align", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, data=2)),
    case("scan_batch.offsets.data_align_double", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, h="scan_d", data=4)),
    case("scan_batch.offsets.ok_total_0", "glu_scan_run_batch_offsets_ptr", lambda c: _scan_off(c, total=0, data=None)),
    # ---- the sort's own entry points, on one object of their own
    case("radix_sort.create.null", "glu_radix_sort_create", lambda c: (None,)),
    case("radix_sort.destroy.null", "glu_radix_sort_destroy", lambda c: (None,)),
    case("radix_sort.prepare.null", "glu_radix_sort_prepare", lambda c: (None, 16)),
    case("radix_sort.prepare.ok_count_0", "glu_radix_sort_prepare", lambda c: (c.h("radix_sort"), 0)),
    case("radix_sort.prepare.ok_count_1", "glu_radix_sort_prepare", lambda c: (c.h("radix_sort"), 1)),
    case("radix_sort.prepare_u64.null", "glu_radix_sort_prepare_u64", lambda c: (None, 16)),
    case("radix_sort.prepare_u64.ok_count_0", "glu_radix_sort_prepare_u64", lambda c: (c.h("radix_sort"), 0)),
    case("radix_sort.prepare_ex.null", "glu_radix_sort_prepare_ex", lambda c: (None, 16, 4, 1)),
    case("radix_sort.prepare_ex.null+key_bytes", "glu_radix_sort_prepare_ex", lambda c: (None, 16, 2, 1)),
    case("radix_sort.prepare_ex.key_bytes", "glu_radix_sort_prepare_ex", lambda c: (c.h("radix_sort"), 16, 2, 1)),
    case("radix_sort.prepare_ex.key_bytes_16", "glu_radix_sort_prepare_ex", lambda c: (c.h("radix_sort"), 16, 16, 0)),
    case("radix_sort.prepare_ex.key_bytes_before_count_0", "glu_radix_sort_prepare_ex", lambda c: (c.h("radix_sort"), 0, 3, 1)),
    case("radix_sort.prepare_ex.ok_count_0", "glu_radix_sort_prepare_ex", lambda c: (c.h("radix_sort"), 0, 8, 0)),
    RS("run_ptr", "null", h=None),
    RS("run_ptr", "null+keys_null", h=None, keys=None),
    RS("run_ptr", "keys_null+vals_null", keys=None, vals=None),
    RS("run_ptr", "keys_null", keys=None),
    RS("run_ptr", "vals_null", vals=None),
    RS("run_ptr", "vals_null+count", vals=None, count=T32),
    RS("run_ptr", "count", count=T32),
    RS("run_ptr", "count+align", count=T32, keys=2),
    RS("run_ptr", "keys_align", keys=2),
    RS("run_ptr", "vals_align", vals=2049),
    RS("run_ptr", "ok_count_0", keys=None, vals=None, count=0),
    RS("run_ptr", "ok_count_1_misaligned_not_looked_at", keys=2, count=1),
    RS("run_u64_ptr", "null", h=None),
    RS("run_u64_ptr", "null+keys_null", h=None, keys=None),
    RS("run_u64_ptr", "keys_null+vals_null", keys=None, vals=None),
    RS("run_u64_ptr", "vals_null", vals=None),
    RS("run_u64_ptr", "count", count=T32),
    RS("run_u64_ptr", "keys_align", keys=4),
    RS("run_u64_ptr", "ok_count_0", keys=None, vals=None, count=0),
    RS("run_keys_ptr", "null", h=None, vals=False),
    RS("run_keys_ptr", "null+keys_null", h=None, keys=None, vals=False),
    RS("run_keys_ptr", "keys_null", keys=None, vals=False),
    RS("run_keys_ptr", "keys_null+count", keys=None, vals=False, count=T32),
    RS("run_keys_ptr", "count", vals=False, count=T32),
    RS("run_keys_ptr", "keys_align", keys=2, vals=False),
    RS("run_keys_ptr", "ok_count_0", keys=None, vals=False, count=0),
    RS("run_keys_u64_ptr", "null", h=None, vals=False),
    RS("run_keys_u64_ptr", "null+keys_null", h=None, keys=None, vals=False),
    RS("run_keys_u64_ptr", "keys_null", keys=None, vals=False),
    RS("run_keys_u64_ptr", "count", vals=False, count=T32),
    RS("run_keys_u64_ptr", "keys_align", keys=4, vals=False),
    RS("run_keys_u64_ptr", "ok_count_0", keys=None, vals=False, count=0),
    RS("run_typed_ptr", "null", h=None, tail=(U32,)),
    RS("run_typed_ptr", "null+key_type", h=None, tail=(BAD_KEY,)),
    RS("run_typed_ptr", "key_type", tail=(6,)),
    RS("run_typed_ptr", "key_type_negative", tail=(-1,)),
    RS("run_typed_ptr", "key_type_before_count_0", count=0, keys=None, tail=(BAD_KEY,)),
    RS("run_typed_ptr", "key_type+keys_null", keys=None, tail=(BAD_KEY,)),
    RS("run_typed_ptr", "keys_null", keys=None, tail=(F64,)),
    RS("run_typed_ptr", "keys_null+count", keys=None, count=T32, tail=(I32,)),
    RS("run_typed_ptr", "count", count=T32, tail=(F32,)),
    RS("run_typed_ptr", "keys_align_u32", keys=2, tail=(I32,)),
    RS("run_typed_ptr", "keys_align_u64", keys=4, tail=(I64,)),
    RS("run_typed_ptr", "ok_count_0", keys=None, vals=None, count=0, tail=(F64,)),
    RS("run_bit_range_ptr", "null", h=None, tail=(32, 0, 32)),
    RS("run_bit_range_ptr", "null+key_bits", h=None, tail=(48, 0, 32)),
    RS("run_bit_range_ptr", "key_bits", tail=(48, 0, 32)),
    RS("run_bit_range_ptr", "key_bits+bit_range", tail=(16, 8, 4)),
    RS("run_bit_range_ptr", "bit_range_order", tail=(32, 8, 4)),
    RS("run_bit_range_ptr", "bit_range_end", tail=(32, 0, 33)),
    RS("run_bit_range_ptr", "bit_range_end_64", tail=(64, 0, 65)),
    RS("run_bit_range_ptr", "bit_range_before_count_0", count=0, keys=None, tail=(32, 0, 33)),
    RS("run_bit_range_ptr", "bit_range+keys_null", keys=None, tail=(32, 8, 4)),
    RS("run_bit_range_ptr", "keys_null", keys=None, tail=(64, 0, 64)),
    RS("run_bit_range_ptr", "keys_null+count", keys=None, count=T32, tail=(32, 0, 32)),
    RS("run_bit_range_ptr", "count", count=T32, tail=(32, 0, 32)),
    RS("run_bit_range_ptr", "keys_align_64", keys=4, tail=(64, 0, 64)),
    RS("run_bit_range_ptr", "ok_count_0", keys=None, vals=None, count=0, tail=(32, 0, 32)),
    RS("run_bit_range_ptr", "ok_no_bits_misaligned_not_looked_at", keys=2, tail=(32, 8, 8)),
    RS("run", "null", _sort_buf, h=None),
    RS("run", "null+key_buffer", _sort_buf, h=None, keys=0),
    RS("run", "key_buffer+value_buffer", _sort_buf, keys=0, vals=0),
    RS("run", "key_buffer", _sort_buf, keys=0),
    RS("run", "key_buffer_unknown", _sort_buf, keys=0x7FFFFFF0),
    RS("run", "value_buffer", _sort_buf, vals=0),
    RS("run", "value_buffer+size", _sort_buf, vals=0, count=1025),
    RS("run", "value_buffer_unknown", _sort_buf, vals=0x7FFFFFF0),
    RS("run", "size", _sort_buf, count=1025),
    RS("run", "size+count", _sort_buf, count=T32),
    RS("run", "ok_count_0", _sort_buf, count=0),
    RS("run", "ok_count_1", _sort_buf, count=1),
    RS("run_u64", "null", _sort_buf, h=None),
    RS("run_u64", "key_buffer+value_buffer", _sort_buf, keys=0, vals=0),
    RS("run_u64", "value_buffer", _sort_buf, vals=0),
    RS("run_u64", "size_keys", _sort_buf, count=513),
    RS("run_u64", "ok_count_0", _sort_buf, count=0),
    RS("run_keys", "null", _sort_buf, h=None, vals=False),
    RS("run_keys", "null+key_buffer", _sort_buf, h=None, keys=0, vals=False),
    RS("run_keys", "key_buffer", _sort_buf, keys=0, vals=False),
    RS("run_keys", "size", _sort_buf, vals=False, count=1025),
    RS("run_keys", "ok_count_0", _sort_buf, vals=False, count=0),
    RS("partition_ptr", "null", _sort_part, h=None),
    RS("partition_ptr", "null+null_array", _sort_part, h=None, sk=None),
    RS("partition_ptr", "src_keys_null", _sort_part, sk=None),
    RS("partition_ptr", "src_vals_null", _sort_part, sv=None),
    RS("partition_ptr", "dst_keys_null", _sort_part, dk=None),
    RS("partition_ptr", "dst_vals_null", _sort_part, dv=None),
    RS("partition_ptr", "null_array+same", _sort_part, sv=None, sk=2048),
    RS("partition_ptr", "same_keys", _sort_part, dk=0),
    RS("partition_ptr", "same_vals", _sort_part, dv=1024),
    RS("partition_ptr", "same+digit", _sort_part, dk=0, bits=0),
    RS("partition_ptr", "digit_bits_0", _sort_part, bits=0),
    RS("partition_ptr", "digit_bits_9", _sort_part, shift=0, bits=9),
    RS("partition_ptr", "digit_past_32", _sort_part, shift=28, bits=8),
    RS("partition_ptr", "digit_before_count_0", _sort_part, sk=None, sv=None, dk=None, dv=None, count=0, bits=0),
    RS("partition_ptr", "digit+count", _sort_part, bits=0, count=T32),
    RS("partition_ptr", "count", _sort_part, count=T32),
    RS("partition_ptr", "ok_count_0", _sort_part, sk=None, sv=None, dk=None, dv=None, count=0),
    RS("run_segments_ptr", "null", _sort_seg, h=None),
    RS("run_segments_ptr", "null+key_bits", _sort_seg, h=None, bits=12),
    RS("run_segments_ptr", "key_bits_12", _sort_seg, bits=12),
    RS("run_segments_ptr", "key_bits_40", _sort_seg, bits=40),
    RS("run_segments_ptr", "key_bits+count", _sort_seg, bits=12, count=T32),
    RS("run_segments_ptr", "count", _sort_seg, count=T32),
    RS("run_segments_ptr", "count+pieces_null", _sort_seg, count=T32, begin=None),
    RS("run_segments_ptr", "piece_begin_null", _sort_seg, begin=None),
    RS("run_segments_ptr", "piece_len_null", _sort_seg, length=None),
    RS("run_segments_ptr", "piece_segment_null", _sort_seg, seg=None),
    RS("run_segments_ptr", "pieces_null+no_segments", _sort_seg, seg=None, nseg=0),
    RS("run_segments_ptr", "no_segments", _sort_seg, nseg=0),
    RS("run_segments_ptr", "segments_max", _sort_seg, nseg=(1 << 24) + 1),
    RS("run_segments_ptr", "segments_max+piece_overruns", _sort_seg, nseg=(1 << 24) + 1, begin=(0, 9)),
    RS("run_segments_ptr", "piece_segment", _sort_seg, seg=(0, 2)),
    RS("run_segments_ptr", "piece_segment+piece_overruns", _sort_seg, seg=(2, 0), begin=(9, 4)),
    RS("run_segments_ptr", "piece_overruns_then_piece_segment", _sort_seg, seg=(0, 2), begin=(9, 4)),
    RS("run_segments_ptr", "piece_begin_overruns", _sort_seg, begin=(0, 9)),
    RS("run_segments_ptr", "piece_len_overruns", _sort_seg, length=(4, 5)),
    RS("run_segments_ptr", "piece_overruns+total", _sort_seg, length=(2, 9)),
    RS("run_segments_ptr", "total_short", _sort_seg, length=(4, 3)),
    RS("run_segments_ptr", "total_long", _sort_seg, begin=(0, 0), length=(4, 8)),
    RS("run_segments_ptr", "total_of_no_pieces", _sort_seg, n=0, begin=None, length=None, seg=None),
    RS("run_segments_ptr", "total+tile", _sort_seg, begin=(0, 0), length=(4, 3)),
    RS("run_segments_ptr", "tile_twice", _sort_seg, begin=(0, 0)),
    RS("run_segments_ptr", "tile_gap", _sort_seg, count=6, begin=(0, 4, 4), length=(2, 2, 2), seg=(0, 1, 1), n=3),
    RS("run_segments_ptr", "tile+null_array", _sort_seg, begin=(0, 0), ik=None),
    RS("run_segments_ptr", "in_keys_null", _sort_seg, ik=None),
    RS("run_segments_ptr", "in_vals_null", _sort_seg, iv=None),
    RS("run_segments_ptr", "out_keys_null", _sort_seg, ok=None),
    RS("run_segments_ptr", "out_vals_null", _sort_seg, ov=None),
    RS("run_segments_ptr", "null_array+same", _sort_seg, iv=None, ok=0),
    RS("run_segments_ptr", "same_keys", _sort_seg, ok=0),
    RS("run_segments_ptr", "same_vals", _sort_seg, ov=1024),
    RS("run_segments_ptr", "ok_count_0", _sort_seg, ik=None, iv=None, ok=None, ov=None, count=0, n=0, begin=None, length=None, seg=None, nseg=0),
    RS("run_segments_ptr", "empty_piece_past_count_0", _sort_seg, ik=None, iv=None, ok=None, ov=None, count=0, length=(0, 0)),
    case("radix_sort.set_digit_bits.null", "glu_radix_sort_set_digit_bits", lambda c: (None, 8)),
    case("radix_sort.set_digit_bits.null+bits", "glu_radix_sort_set_digit_bits", lambda c: (None, 5)),
    case("radix_sort.set_digit_bits.bits_5", "glu_radix_sort_set_digit_bits", lambda c: (c.h("radix_sort"), 5)),
    case("radix_sort.set_digit_bits.bits_0", "glu_radix_sort_set_digit_bits", lambda c: (c.h("radix_sort"), 0)),
    case("radix_sort.set_digit_bits.ok_4", "glu_radix_sort_set_digit_bits", lambda c: (c.h("radix_sort"), 4)),
    case("radix_sort.set_digit_bits.ok_8", "glu_radix_sort_set_digit_bits", lambda c: (c.h("radix_sort"), 8)),
    case("radix_sort.get_digit_bits.null", "glu_radix_sort_get_digit_bits", lambda c: (None, c.ref(c.word))),
    case("radix_sort.get_digit_bits.null+bits_null", "glu_radix_sort_get_digit_bits", lambda c: (None, None)),
    case("radix_sort.get_digit_bits.bits_null", "glu_radix_sort_get_digit_bits", lambda c: (c.h("radix_sort"), None)),
    case("radix_sort.get_digit_bits.ok", "glu_radix_sort_get_digit_bits", lambda c: (c.h("radix_sort"), c.ref(c.word))),
    case("radix_sort.set_option.null", "glu_radix_sort_set_option", lambda c: (None, b"SORT_NO_PLAN", 0)),
    case("radix_sort.set_option.null+name_null", "glu_radix_sort_set_option", lambda c: (None, None, 0)),
    case("radix_sort.set_option.name_null", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), None, 0)),
    case("radix_sort.set_option.unknown", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"SORT_FASTER", 1)),
    case("radix_sort.set_option.unknown_prefix_only", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"GLU_HIP_", 1)),
    case("radix_sort.set_option.unknown_empty", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"", 1)),
    case("radix_sort.set_option.ok", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"SORT_NO_PLAN", 0)),
    case("radix_sort.set_option.ok_environment_spelling", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"glu_hip_sort_no_plan", 0)),
    case("radix_sort.set_option.ok_digit_bits_5_ignored", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"DIGIT_BITS", 5)),
    case("radix_sort.set_option.ok_sort_blocks_negative_ignored", "glu_radix_sort_set_option", lambda c: (c.h("radix_sort"), b"SORT_BLOCKS", -1)),
    case("radix_sort.scratch_size.null", "glu_radix_sort_scratch_size", lambda c: (None, c.ref(c.size))),
    case("radix_sort.scratch_size.null+bytes_null", "glu_radix_sort_scratch_size", lambda c: (None, None)),
    case("radix_sort.scratch_size.bytes_null", "glu_radix_sort_scratch_size", lambda c: (c.h("radix_sort"), None)),
    case("radix_sort.scratch_size.ok", "glu_radix_sort_scratch_size", lambda c: (c.h("radix_sort"), c.ref(c.size))),
    host("radix_sort.scratch_placement.null", "glu_radix_sort_scratch_placement", lambda c: (None, None, None, None)),
    case("radix_sort.scratch_placement.ok_outs_null", "glu_radix_sort_scratch_placement", lambda c: (c.h("radix_sort"), None, None, None)),
    case("radix_sort.read_plan.null", "glu_radix_sort_read_plan", lambda c: (None, None, None, None, 4)),
    case("radix_sort.read_plan.null+passes", "glu_radix_sort_read_plan", lambda c: (None, None, None, None, 33)),
    case("radix_sort.read_plan.passes+no_sort", "glu_radix_sort_read_plan", lambda c: (c.h("radix_sort"), None, None, None, 33)),
    case("radix_sort.read_plan.no_sort", "glu_radix_sort_read_plan", lambda c: (c.h("radix_sort"), None, None, None, 32)),
    case("radix_sort.read_plan.no_sort_no_passes", "glu_radix_sort_read_plan", lambda c: (c.h("radix_sort"), None, None, None, 0)),
    case("radix_sort.read_finish.null", "glu_radix_sort_read_finish", lambda c: (None,) * 6),
    case("radix_sort.read_finish.ok_no_sort", "glu_radix_sort_read_finish", lambda c: (c.h("radix_sort"),) + (None,) * 5),
    case("radix_sort.read_long_runs.null", "glu_radix_sort_read_long_runs", lambda c: (None,) * 4),
    case("radix_sort.read_long_runs.ok_no_sort", "glu_radix_sort_read_long_runs", lambda c: (c.h("radix_sort"),) + (None,) * 3),
    case("radix_sort.read_seg_finish.null", "glu_radix_sort_read_seg_finish", lambda c: (None,) * 8),
    case("radix_sort.read_seg_finish.ok_no_sort", "glu_radix_sort_read_seg_finish", lambda c: (c.h("radix_sort"),) + (None,) * 7),
    case("radix_sort.read_profile.null", "glu_radix_sort_read_profile", lambda c: (None,) * 5),
    case("radix_sort.read_profile.ok_no_sort", "glu_radix_sort_read_profile", lambda c: (c.h("radix_sort"),) + (None,) * 4),
    case("radix_sort.read_profile_finish.null", "glu_radix_sort_read_profile_finish", lambda c: (None,) * 7),
    case("radix_sort.read_profile_finish.ok_no_sort", "glu_radix_sort_read_profile_finish", lambda c: (c.h("radix_sort"),) + (None,) * 6),
    case("radix_sort.set_profiling.null", "glu_radix_sort_set_profiling", lambda c: (None, 1)),
    case("radix_sort.set_profiling.ok_off", "glu_radix_sort_set_profiling", lambda c: (c.h("radix_sort"), 0)),
    # ---- the sort's plan entry points
    plan("radix_sort.plan_finish.key_bytes", "glu_radix_sort_plan_finish", 1 << 28, 2),
    plan("radix_sort.plan_finish.key_bytes_before_count_0", "glu_radix_sort_plan_finish", 0, 16),
    plan("radix_sort.plan_finish.ok", "glu_radix_sort_plan_finish", 1 << 28, 4),
    plan("radix_sort.plan_finish.ok_wide", "glu_radix_sort_plan_finish", 1 << 24, 8),
    plan("radix_sort.plan_finish.ok_no_attempt", "glu_radix_sort_plan_finish", 1 << 20, 4),
    plan("radix_sort.plan_finish.ok_count_0", "glu_radix_sort_plan_finish", 0, 4),
    host("radix_sort.plan_segments.piece_begin_null", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, begin=None)),
    host("radix_sort.plan_segments.piece_len_null", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, length=None)),
    host("radix_sort.plan_segments.piece_segment_null", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, seg=None)),
    host("radix_sort.plan_segments.pieces_null+workgroups_0", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, seg=None, nwg=0)),
    host("radix_sort.plan_segments.workgroups_0", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, nwg=0)),
    host("radix_sort.plan_segments.num_sub_blocks_null", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, num=False)),
    host("radix_sort.plan_segments.workgroups_0+segments_max", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, nwg=0, nseg=(1 << 24) + 1)),
    host("radix_sort.plan_segments.segments_max", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, nseg=(1 << 24) + 1)),
    host("radix_sort.plan_segments.segments_max+workgroups_max", "glu_radix_sort_plan_segments",
         lambda c: _plan_seg(c, nseg=(1 << 24) + 1, nwg=(1 << 20) + 1)),
    host("radix_sort.plan_segments.workgroups_max", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, nwg=(1 << 20) + 1)),
    host("radix_sort.plan_segments.workgroups_max+piece_segment", "glu_radix_sort_plan_segments",
         lambda c: _plan_seg(c, nwg=(1 << 20) + 1, seg=(0, 2))),
    host("radix_sort.plan_segments.piece_segment", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, seg=(0, 2))),
    host("radix_sort.plan_segments.no_segments", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, nseg=0)),
    host("radix_sort.plan_segments.piece_segment+total", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, seg=(2, 0), length=(0xFFFF0000, 1))),
    host("radix_sort.plan_segments.total", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, length=(0xFFFF0000, 1))),
    host("radix_sort.plan_segments.room", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, cap=0)),
    host("radix_sort.plan_segments.ok", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c)),
    host("radix_sort.plan_segments.ok_pieces_overlap_not_looked_at", "glu_radix_sort_plan_segments", lambda c: _plan_seg(c, begin=(0, 0))),
    host("radix_sort.plan_segments.ok_no_pieces", "glu_radix_sort_plan_segments",
         lambda c: _plan_seg(c, n=0, begin=None, length=None, seg=None, nseg=0)),
    # ---- the sharded sort: its plan calls, and every handle check (no object: making one needs RCCL)
    host("dist.plan_buckets.hist_null", "glu_dist_plan_buckets", lambda c: (None, 2, c.owner)),
    host("dist.plan_buckets.owner_null", "glu_dist_plan_buckets", lambda c: (c.hist, 2, None)),
    host("dist.plan_buckets.world_0", "glu_dist_plan_buckets", lambda c: (c.hist, 0, c.owner)),
    host("dist.plan_buckets.ok", "glu_dist_plan_buckets", lambda c: (c.hist, 2, c.owner)),
    host("dist.plan_counts.hist_null", "glu_dist_plan_counts", lambda c: (None, 2, 0, c.owner, c.send, c.recv)),
    host("dist.plan_counts.owner_null", "glu_dist_plan_counts", lambda c: (c.hist, 2, 0, None, c.send, c.recv)),
    host("dist.plan_counts.send_null", "glu_dist_plan_counts", lambda c: (c.hist, 2, 0, c.owner, None, c.recv)),
    host("dist.plan_counts.recv_null", "glu_dist_plan_counts", lambda c: (c.hist, 2, 0, c.owner, c.send, None)),
    host("dist.plan_counts.world_0", "glu_dist_plan_counts", lambda c: (c.hist, 0, 0, c.owner, c.send, c.recv)),
    host("dist.plan_counts.rank_negative", "glu_dist_plan_counts", lambda c: (c.hist, 2, -1, c.owner, c.send, c.recv)),
    host("dist.plan_counts.rank_is_world", "glu_dist_plan_counts", lambda c: (c.hist, 2, 2, c.owner, c.send, c.recv)),
    host("dist.plan_counts.rank+owner", "glu_dist_plan_counts", lambda c: (c.hist, 2, 2, c.owner_high, c.send, c.recv)),
    host("dist.plan_counts.owner_high", "glu_dist_plan_counts", lambda c: (c.hist, 2, 1, c.owner_high, c.send, c.recv)),
    host("dist.plan_counts.owner_negative", "glu_dist_plan_counts", lambda c: (c.hist, 2, 1, c.owner_negative, c.send, c.recv)),
    host("dist.plan_counts.owner_is_world", "glu_dist_plan_counts", lambda c: (c.hist, 1, 0, c.owner, c.send, c.recv)),
    host("dist.plan_counts.ok", "glu_dist_plan_counts", lambda c: (c.hist, 2, 1, c.owner, c.send, c.recv)),
    host("dist.plan_groups.hist_null", "glu_dist_plan_groups", lambda c: (None, 2, c.owner, 2, c.cut)),
    host("dist.plan_groups.owner_null", "glu_dist_plan_groups", lambda c: (c.hist, 2, None, 2, c.cut)),
    host("dist.plan_groups.cut_null", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner, 2, None)),
    host("dist.plan_groups.world_0", "glu_dist_plan_groups", lambda c: (c.hist, 0, c.owner, 2, c.cut)),
    host("dist.plan_groups.rounds_0", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner, 0, c.cut)),
    host("dist.plan_groups.rounds_9", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner, 9, c.cut)),
    host("dist.plan_groups.rounds+owner", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner_high, 9, c.cut)),
    host("dist.plan_groups.owner_high", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner_high, 2, c.cut)),
    host("dist.plan_groups.owner_negative", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner_negative, 8, c.cut)),
    host("dist.plan_groups.ok", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner, 2, c.cut)),
    host("dist.plan_groups.ok_rounds_8", "glu_dist_plan_groups", lambda c: (c.hist, 2, c.owner, 8, c.cut)),
    host("dist.destroy.null", "glu_dist_destroy", lambda c: (None,)),
    host("dist.partition_shift.null", "glu_dist_partition_shift", lambda c: (None, c.ref(c.word))),
    host("dist.partition_shift.null+shift_null", "glu_dist_partition_shift", lambda c: (None, None)),
    host("dist.world.null", "glu_dist_world", lambda c: (None, None, None)),
    host("dist.local_sorter.null", "glu_dist_local_sorter", lambda c: (None, c.ref(c.tmp))),
    host("dist.local_sorter.null+out_null", "glu_dist_local_sorter", lambda c: (None, None)),
    host("dist.set_profiling.null", "glu_dist_set_profiling", lambda c: (None, 1)),
    host("dist.set_rounds.null", "glu_dist_set_rounds", lambda c: (None, 2)),
    host("dist.set_rounds.null+rounds", "glu_dist_set_rounds", lambda c: (None, 9)),
    host("dist.last_rounds.null", "glu_dist_last_rounds", lambda c: (None, c.ref(c.word))),
    host("dist.last_rounds.null+rounds_null", "glu_dist_last_rounds", lambda c: (None, None)),
    host("dist.last_local_sort.null", "glu_dist_last_local_sort", lambda c: (None, c.ref(c.word))),
    host("dist.last_local_sort.null+segmented_null", "glu_dist_last_local_sort", lambda c: (None, None)),
    case("dist.prepare.null", "glu_dist_prepare", lambda c: (None, 16, 16)),
    case("dist.set_reserved_cus.null", "glu_dist_set_reserved_cus", lambda c: (None, 8)),
    case("dist.set_reserved_cus.null+cus", "glu_dist_set_reserved_cus", lambda c: (None, -1)),
    case("dist.phase_times.null", "glu_dist_phase_times", lambda c: (None, None, None)),
    case("dist.sort_begin.null", "glu_dist_sort_begin", lambda c: (None, c.A, c.A + 2048, 16, None, c.ref(c.size))),
    case("dist.sort_begin.null+arrays_null", "glu_dist_sort_begin", lambda c: (None, None, None, 16, None, None)),
    case("dist.sort_finish.null", "glu_dist_sort_finish", lambda c: (None, c.A, c.A + 2048, 16, None)),
    case("dist.sort_ptr.null", "glu_dist_sort_ptr", lambda c: (None, c.A, c.A + 2048, 16, None, None, None, None)),
]


def _outs(fn, given):
    """ctypes objects for the out-parameters that follow the `given` leading arguments of a plan entry point"""
    return [t._type_() for t in fn.argtypes[given:]]


def run_case(c, k):
    """{status, message, out (plan entry points), last (units that have one)} of one case"""
    fn = getattr(c.L, k["fn"])
    args = k["args"](c)
    rec = {}
    if not k["gpu"]:
        outs = _outs(fn, len(args))
        rec["status"] = fn(*args, *[ctypes.byref(o) for o in outs])
        rec["out"] = [int(o.value) for o in outs] if rec["status"] == 0 else None
        if rec["status"] == 0:  # the same call with every out-parameter NULL is accepted too
            assert fn(*args, *[None] * len(outs)) == 0, k["name"]
    else:
        rec["status"] = fn(*args)
    rec["message"] = c.L.glu_last_error().decode() if rec["status"] else ""
    unit = k["name"].split(".")[0]
    if k["gpu"] and unit in LAST:
        name, words = LAST[unit]
        out = [ctypes.c_uint32() for _ in range(words)]
        c.G.check(getattr(c.L, name)(c.h(unit), *[ctypes.byref(o) for o in out]))
        rec["last"] = [o.value for o in out]
    return rec


def record(G, gpu):
    """{name: record} of the plan cases (gpu False) or the object cases (gpu True), in the table's order"""
    c = Ctx(G)
    try:
        got = {k["name"]: run_case(c, k) for k in CASES if k["gpu"] == gpu}
        if gpu:
            G.synchronize()  # (the accepted cases enqueue kernels)
    finally:
        c.close()
    return got


def _compare(got, want):
    assert list(got) == [n for n in want if n in got], "the table and the record name the same cases in the same order"
    wrong = ["%s:\n  recorded %r\n  now      %r" % (n, want.get(n), got[n]) for n in got if got[n] != want.get(n)]
    assert not wrong, "%d of %d calls answer differently:\n%s" % (len(wrong), len(got), "\n".join(wrong))


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_and_record_name_the_same_cases(recorded):
    names = [k["name"] for k in CASES]
    assert len(set(names)) == len(names)
    assert names == list(recorded)
    assert all("0x" not in r["message"] for r in recorded.values()), "no message holds an address"
    accepted = [n for n, r in recorded.items() if r["status"] == 0]
    assert all(".ok" in n or ".destroy.null" in n or "adjacent" in n or "not_looked_at" in n for n in accepted), accepted
    assert all(r["status"] == 0 for n, r in recorded.items() if ".ok" in n or "adjacent" in n or "not_looked_at" in n)


def test_plan_refusals(built, recorded):
    _compare(record(built, gpu=False), recorded)


@pytest.mark.gpu
def test_object_refusals(built, recorded):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _compare(record(built, gpu=True), recorded)
