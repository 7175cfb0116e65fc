"""Random call sequences on long-lived operator objects, and their numpy answers (a plain module: nothing here is collected).

sequence(unit, seed, steps) draws a list of fully specified calls on ONE set of objects of a unit: every scalar argument, every host
array, every alignment shift, the options to set before the call.  expected(step) is the numpy answer for one step: the contents of
every array the call may write, with poison wherever the header says the call leaves the array alone.  check(step, images) compares
the bytes that came back from the device, guards included, with that answer.  run_sequence() is the device side; it is only called
from the GPU tests.  The order of the steps is the point: a small call after a large one, another key width, other optional outputs,
on an object whose device-resident scratch still holds what the earlier call left there.

An object of BlellochScan and Reduce is bound to its data type (and operator) when it is created, so a sequence of those units holds
three long-lived objects and alternates between them; every other unit is a single object (KeyRuns: the runs object and the Reduce and
BlellochScan it feeds).  Class and tile edges come from the host-only plan functions of the binding, never from constants here.

Everything is compared on bits.  Floats that are summed are small integers, floats that are multiplied are +-1 with at most twenty
factors of two, so every order of combination gives the same bits."""
import hashlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gl-radix-sort_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_top_k_pick import key_code  # noqa: E402

UNITS = ["RadixSort", "BlellochScan", "Reduce", "KeyRuns", "Select", "SortedSearch", "Merge", "SetOps", "Histogram", "Expand", "Gather",
         "TopK"]
SEEDS = {unit: (101 + 2 * i, 102 + 2 * i) for i, unit in enumerate(UNITS)}  # the committed seeds, two per unit
STEPS = 40
GUARD = 64  # bytes of poison in front of and behind every array, inside its allocation (a multiple of 16)
POISON = 0xA5
KEY_TYPES = ("uint32", "int32", "float32", "uint64", "int64", "float64")
TINY = (0, 1, 2, 63, 64, 65)
# glu_data_type -> (numpy scalar type, components); the table of oracle.dtype_info, restated so that this module needs no oracle build
DATA_TYPES = {0: ("float32", 1), 1: ("float64", 1), 2: ("int32", 1), 3: ("uint32", 1), 4: ("float32", 2), 5: ("float32", 4),
              6: ("float64", 2), 7: ("float64", 4), 8: ("uint32", 2), 9: ("uint32", 4), 10: ("int32", 2), 11: ("int32", 4)}
SUM, MUL, MIN, MAX = range(4)


def G():
    import glu_hip

    glu_hip.lib()
    return glu_hip


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------- arrays and steps


def uint_of(dtype):
    return np.dtype("uint%d" % (8 * np.dtype(dtype).itemsize))


def poisoned(n, dtype):
    """n elements of `dtype` whose every byte is POISON: an output array before the call."""
    dt = np.dtype(dtype)
    return np.full(n * dt.itemsize, POISON, dtype=np.uint8).view(dt)


def arr_in(data, shift=0):
    return {"data": np.ascontiguousarray(data), "role": "in", "shift": int(shift)}


def arr_out(n, dtype, shift=0):
    return {"data": poisoned(n, dtype), "role": "out", "shift": int(shift)}


def arr_inout(data, shift=0, carry=False):
    return {"data": np.ascontiguousarray(data), "role": "inout", "shift": int(shift), "carry": carry}


def draw_shift(rng, elem_bytes):
    """Bytes behind a 16-byte boundary: a multiple of the alignment the header asks for (the element size, 16 at most)."""
    a = min(elem_bytes, 16)
    return int(rng.integers(0, 16 // a)) * a


def image(a, content=None):
    """The bytes of the allocation of array `a`: guard, shift, contents (`content` in place of the step's own), guard."""
    body = np.ascontiguousarray(a["data"] if content is None else content).view(np.uint8).ravel()
    assert body.size == a["data"].nbytes
    return np.concatenate([np.full(GUARD + a["shift"], POISON, dtype=np.uint8), body, np.full(GUARD, POISON, dtype=np.uint8)])


def scalars(step):
    return (step["unit"], step["seed"], step["index"], step["call"], step["args"], step["options"])


def expected_images(step):
    want = expected(step)
    return {name: image(a, want.get(name) if a["role"] != "in" else None) for name, a in step["arrays"].items()}


def check(step, images, diag=None):
    """Raises Mismatch unless every allocation that came back equals the numpy answer byte for byte (guards, the room the call must
    leave alone and the inputs included) and the object's own account of the call (`diag`) is the plan's."""
    want = expected_images(step)
    for name, a in step["arrays"].items():
        got, exp = np.asarray(images[name]).view(np.uint8), want[name]
        if got.size != exp.size:
            raise Mismatch("%r: array %s came back with %d bytes, not %d" % (scalars(step), name, got.size, exp.size))
        bad = np.flatnonzero(got != exp)
        if bad.size:
            at = int(bad[0]) - GUARD - a["shift"]
            where = "guard" if at < 0 or at >= a["data"].nbytes else "input" if a["role"] == "in" else "contents"
            lo = int(bad[0]) // 8 * 8
            raise Mismatch("%r: array %s differs in its %s, first at byte %d of %d (%d bytes differ, the last at byte %d): got %s, numpy %s"
                           % (scalars(step), name, where, at, a["data"].nbytes, bad.size, int(bad[-1]) - GUARD - a["shift"],
                              got[lo:lo + 16].tobytes().hex(), exp[lo:lo + 16].tobytes().hex()))
    if diag is not None:
        exp = expected_diag(step)
        for key, value in exp.items():
            if diag.get(key) != value:
                raise Mismatch("%r: the object reports %s = %r, the plan says %r" % (scalars(step), key, diag.get(key), value))


def step_hash(steps):
    """A hash of everything drawn: scalars, options and the bytes and shifts of every array."""
    h = hashlib.sha256()
    for s in steps:
        h.update(repr((s["call"], s["obj"], sorted(s["args"].items()), s["options"], s["size"], s["type"], s["variant"])).encode())
        for name in sorted(s["arrays"]):
            a = s["arrays"][name]
            h.update(repr((name, a["role"], a["shift"], str(a["data"].dtype), a.get("carry", False))).encode())
            h.update(np.ascontiguousarray(a["data"]).view(np.uint8).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- drawing


def last_where(pred, hi=1 << 40):
    """The largest c >= 0 with pred(c), for a pred that holds up to a point and not beyond it."""
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def draw_size(rng, i, cap, edges):
    """Step i's size: the three sources of the issue in a fixed rotation, so that small calls follow large ones in every sequence."""
    kind = ("log", "big", "small", "edge", "tiny")[i % 5]
    if kind == "big":
        n = int(cap * 2.0 ** rng.uniform(-1, 0))
    elif kind == "tiny":
        n = int(rng.choice(TINY, p=(0.25, 0.15, 0.15, 0.15, 0.15, 0.15)))
    elif kind == "small":
        n = int(2.0 ** rng.uniform(0, math.log2(max(2, cap // 16))))
    elif kind == "edge" and len(edges):
        n = int(rng.choice(sorted(edges))) + int(rng.integers(-1, 2))
    else:
        n = int(2.0 ** rng.uniform(0, math.log2(cap)))
    return max(0, min(n, cap))


def draw_other(rng, choices, prev, force):
    """One of `choices`; another one than `prev` when `force` (and there is another)."""
    choices = list(choices)
    for _ in range(64):
        c = choices[int(rng.integers(0, len(choices)))]
        if not force or c != prev or len(choices) == 1:
            return c
    return c


def draw_lengths(rng, budget, edges, most=200):
    """Segment lengths that sum to at most `budget`: zeros, ones, short ones, lengths at the class edges -1 / 0 / +1, long ones."""
    lens, left = [0], int(budget)
    edges = sorted(e for e in edges if e > 0)
    while left > 0 and len(lens) < most:
        kind = int(rng.integers(0, 6))
        if kind == 0:
            n = 0
        elif kind == 1:
            n = int(rng.integers(1, 4))
        elif kind == 2:
            n = int(rng.geometric(1 / 40.0))
        elif kind in (3, 4) and edges:
            n = max(0, int(rng.choice(edges)) + int(rng.integers(-1, 2)))
        else:
            n = int(2.0 ** rng.uniform(0, math.log2(max(2, left))))
        n = min(n, left)
        lens.append(n)
        left -= n
    lens = np.array(lens, dtype=np.int64)
    rng.shuffle(lens)
    return lens


def offsets_from(rng, lens):
    """(offsets, total): the segments start behind a few loose elements and a few follow them."""
    head, tail = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    offsets = head + np.concatenate([[0], np.cumsum(lens)])
    return offsets.astype(np.uint32), int(offsets[-1]) + tail


def draw_keys(rng, key_type, n):
    """n keys of `key_type` out of a pool of bit patterns of a drawn size, so that ties are heavy in some steps and rare in others;
    floats: NaNs of both signs with two payloads, +-0, +-inf and denormals are in the pool."""
    dt = np.dtype(key_type)
    u = uint_of(dt)
    width = 8 * dt.itemsize
    m = int(rng.choice([3, 17, n // 4 + 1, 4 * n + 8]))
    pool = rng.integers(0, 2 ** width, m, dtype=u)
    if dt.kind == "f":
        sign = 1 << (width - 1)
        nan = int(np.array([np.nan], dtype=dt).view(u)[0])
        inf = int(np.array([np.inf], dtype=dt).view(u)[0])
        special = [0, sign, inf, inf | sign, nan, nan | sign, nan | 1, nan | sign | 5, 1, sign | 1, 3, sign | 7]
        where = rng.permutation(m)[:min(m, len(special)) if m > 3 else 1]
        pool[where] = np.array(special, dtype=u)[rng.permutation(len(special))[:where.size]]
    return pool[rng.integers(0, m, n)].view(dt)


def in_sort_order(keys):
    return keys[np.argsort(key_code(keys, False), kind="stable")]


def new_step(unit, seed, index, call, obj, args, arrays, size, type_, variant, options=()):
    return {"unit": unit, "seed": seed, "index": index, "call": call, "obj": obj, "args": args, "arrays": arrays, "size": int(size),
            "type": type_, "variant": variant, "options": list(options)}


# ---------------------------------------------------------------------------------------------------------------- RadixSort (batched)


def sort_edges(g, key_type, with_vals):
    kb = np.dtype(key_type).itemsize
    wave = last_where(lambda c: g.plan_batch(c, kb, with_vals)[0] <= 1)
    block = last_where(lambda c: g.plan_batch(c, kb, with_vals)[0] <= 2)
    tiles = sorted({g.plan_batch(c, kb, with_vals)[1] for c in (wave + 1, block // 8, block // 2, block)})
    return wave, block, tiles


def gen_radix_sort(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    for i in range(steps):
        key_type = draw_other(rng, KEY_TYPES, prev_type, i % 2 == 1)
        dt, kb = np.dtype(key_type), np.dtype(key_type).itemsize
        calls = ["sort_batch_offsets_ptr", "sort_batch_offsets_ptr", "sort_batch_ptr", "sort_typed_ptr", "sort_bit_range_ptr"]
        if dt.kind == "u":
            calls.append("sort_keys_ptr")
        call, with_vals = draw_other(rng, [(c, v) for c in calls for v in (True, False) if not (v and c == "sort_keys_ptr")], prev_variant,
                                     i % 3 == 0)
        if i % 10 == 1:  # a large step of equal partitions beyond the single-block limit
            call = "sort_batch_ptr"
        wave, block, tiles = sort_edges(g, key_type, with_vals)
        edges = [wave, block] + tiles
        size = draw_size(rng, i, cap, edges + [cap - 1])
        args, arrays = {"key_type": key_type, "with_vals": with_vals}, {}
        if call == "sort_batch_offsets_ptr":
            lens = draw_lengths(rng, size, edges)
            offsets, total = offsets_from(rng, lens)
            args.update(total=total, num_segments=int(lens.size))
            arrays["offsets"] = arr_in(offsets, draw_shift(rng, 4))
        elif call == "sort_batch_ptr":
            count = max(1, min(size, int(rng.choice(edges + [1, 2, 3, 100, size // 2, size // 3])) + int(rng.integers(-1, 2)))) if size else 0
            if i % 10 == 1:
                count = size // int(rng.integers(1, 4))
            parts = min(size // count, 2000) if count else int(rng.integers(0, 3))
            args.update(count=count, num_partitions=int(parts))
            total = count * parts
        else:
            total = max(1, size)
            args.update(count=total)
            if call == "sort_bit_range_ptr":
                b = int(rng.integers(0, 8 * kb))
                args.update(begin_bit=b, end_bit=int(rng.integers(b + 1, 8 * kb + 1)))
        arrays["keys"] = arr_inout(draw_keys(rng, key_type, total), draw_shift(rng, kb))
        if with_vals:
            arrays["vals"] = arr_inout(rng.integers(0, 2 ** 32, total, dtype=np.uint32), draw_shift(rng, 4))
        out.append(new_step(unit, seed, i, call, "sort", args, arrays, total, key_type, (call, with_vals)))
        prev_type, prev_variant = key_type, (call, with_vals)
    return out


def sort_segments(step):
    a = step["args"]
    if step["call"] == "sort_batch_offsets_ptr":
        o = step["arrays"]["offsets"]["data"].astype(np.int64)
        return list(zip(o[:-1], o[1:]))
    if step["call"] == "sort_batch_ptr":
        return [(p * a["count"], (p + 1) * a["count"]) for p in range(a["num_partitions"])]
    return [(0, a["count"])]


def exp_radix_sort(step):
    a, arrays = step["args"], step["arrays"]
    keys = arrays["keys"]["data"]
    vals = arrays["vals"]["data"] if "vals" in arrays else None
    if step["call"] in ("sort_typed_ptr", "sort_batch_offsets_ptr", "sort_batch_ptr"):
        code = key_code(keys, False)
    else:  # untyped words, all their bits or a range of them
        code = keys.view(uint_of(keys.dtype)).copy()
        if step["call"] == "sort_bit_range_ptr":
            u = code.dtype.type
            width = a["end_bit"] - a["begin_bit"]
            mask = u((1 << width) - 1)
            code = (code >> u(a["begin_bit"])) & mask
    ek, ev = keys.copy(), None if vals is None else vals.copy()
    for b, e in sort_segments(step):
        order = np.argsort(code[b:e], kind="stable")
        ek[b:e] = keys[b:e][order]
        if vals is not None:
            ev[b:e] = vals[b:e][order]
    out = {"keys": ek}
    if vals is not None:
        out["vals"] = ev
    return out


def batch_classes(lengths, path_of, skip):
    got = {"wave": 0, "block": 0, "long": 0}
    for n in lengths:
        if n > skip:
            got[("wave", "block", "long")[path_of(int(n)) - 1]] += 1
    return got


def diag_radix_sort(step):
    if not step["call"].startswith("sort_batch"):
        return {}
    g, a = G(), step["args"]
    kb = np.dtype(a["key_type"]).itemsize
    lens = [e - b for b, e in sort_segments(step)]
    return batch_classes(lens, lambda n: g.plan_batch(n, kb, a["with_vals"])[0], 1)


def classes_radix_sort(step):
    g, a = G(), step["args"]
    kb = np.dtype(a["key_type"]).itemsize
    if not step["call"].startswith("sort_batch"):
        return ["single:" + step["call"]]
    tiles = sort_edges(g, a["key_type"], a["with_vals"])[2]
    form = "offsets" if step["call"] == "sort_batch_offsets_ptr" else "equal"
    out = set()
    for b, e in sort_segments(step):
        path, tile = g.plan_batch(int(e - b), kb, a["with_vals"])
        if path == 2:
            out.add("%s:block:tile%d" % (form, tiles.index(tile)) if form == "offsets" else "equal:block")
        elif path:
            out.add("%s:%s" % (form, "wave" if path == 1 else "long"))
    return sorted(out)


def required_radix_sort():
    return ["offsets:wave", "offsets:block:tile0", "offsets:block:tile1", "offsets:block:tile2", "offsets:long", "equal:wave",
            "equal:block", "equal:long", "single:sort_typed_ptr", "single:sort_keys_ptr", "single:sort_bit_range_ptr"]


# ---------------------------------------------------------------------------------------------------------------- Reduce and Scan data


def elem_bytes(dt):
    name, comps = DATA_TYPES[dt]
    return np.dtype(name).itemsize * comps


def reduce_edges(plan, es):
    """The lengths at which a batched scan or reduce changes its class or its lane group, and two and three chunks of the long class."""
    wave = last_where(lambda c: plan(c, es)[0] <= 1)
    block = last_where(lambda c: plan(c, es)[0] <= 2)
    chunk = last_where(lambda c: c <= block or plan(c, es)[1] <= plan(block + 1, es)[1]) // max(1, plan(block + 1, es)[1])
    return wave, block, chunk


def draw_values(rng, dt, op, rows, segments):
    """rows x components scalars of data type dt that `op` combines exactly in any order."""
    name, comps = DATA_TYPES[dt]
    npdt = np.dtype(name)
    if npdt.kind != "f":
        return rng.integers(0, 2 ** 32, rows * comps, dtype=np.uint32).view(npdt)
    if op == MUL:
        d = rng.choice(np.array([1.0, -1.0]), (rows, comps))
        for b, e in segments:
            if e > b:
                at = b + rng.integers(0, e - b, min(20, e - b))
                at = np.unique(at)
                d[at] *= rng.choice(np.array([2.0, 0.5]), (at.size, 1))
        return d.astype(npdt).reshape(-1)
    return rng.integers(-8, 9, rows * comps).astype(npdt)  # (an integer never becomes -0.0)


def identity_of(npdt, op):
    npdt = np.dtype(npdt)
    if op == SUM:
        return npdt.type(0)
    if op == MUL:
        return npdt.type(1)
    if npdt.kind == "f":
        return npdt.type(np.inf if op == MIN else -np.inf)
    info = np.iinfo(npdt)
    return npdt.type(info.max if op == MIN else info.min)


def fold(rows, op, order="forward"):
    """`op` over the rows of a 2-D array of one segment, in the array's own type (signed sums and products wrap through an unsigned
    view, as the device's do), forwards, backwards or as a balanced tree."""
    npdt = rows.dtype
    work = rows.view(np.uint32) if npdt.kind == "i" and op in (SUM, MUL) else rows
    f = (np.add, np.multiply, np.minimum, np.maximum)[op]
    if work.shape[0] == 0:
        return np.full(work.shape[1:], identity_of(work.dtype, op), dtype=work.dtype).view(npdt)
    with np.errstate(over="ignore"):
        if order == "pairwise":
            while work.shape[0] > 1:
                if work.shape[0] % 2:
                    work = np.concatenate([work, np.full((1,) + work.shape[1:], identity_of(work.dtype, op), dtype=work.dtype)])
                work = f(work[0::2], work[1::2])
            return np.ascontiguousarray(work[0]).view(npdt)
        if order == "backward":
            work = work[::-1]
        return np.asarray(f.reduce(work, axis=0), dtype=work.dtype).view(npdt)


def exclusive_scan(rows, order="forward"):
    """Exclusive + scan down the rows of one segment, in the array's own type: every prefix added up from its front, or ("backward")
    taken as the total less the suffix that was added up from the far end."""
    npdt = rows.dtype
    work = rows.view(np.uint32) if npdt.kind in "iu" else rows
    out = np.zeros_like(work)
    if work.shape[0] > 1:
        with np.errstate(over="ignore"):
            if order == "forward":
                np.cumsum(work[:-1], axis=0, dtype=work.dtype, out=out[1:])
            else:
                suffix = np.cumsum(work[::-1], axis=0, dtype=work.dtype)[::-1]  # suffix[i] = work[i] + ... + work[n - 1]
                out[1:] = suffix[0] - suffix[1:]
    return out.view(npdt)


# ---------------------------------------------------------------------------------------------------------------- Reduce


def gen_reduce(g, rng, unit, seed, steps):
    dts = [int(x) for x in rng.permutation(12)[:4]]
    if len({elem_bytes(d) for d in dts}) < 2:
        dts[0] = 7 if elem_bytes(dts[1]) != 32 else 3
    pool = [(dt, int(op)) for dt, op in zip(dts, rng.permutation(4))] + [(dts[0], int(rng.integers(0, 4)))]
    pool = list(dict.fromkeys(pool))
    out, prev, prev_call = [], None, None
    for i in range(steps):
        dt, op = draw_other(rng, [p for p in pool if i % 2 == 0 or prev is None or p[0] != prev[0]], prev, True)
        call = draw_other(rng, ["run_batch_offsets_ptr", "run_batch_offsets_ptr", "run_batch_ptr"], prev_call, i % 3 == 0)
        es = elem_bytes(dt)
        name, comps = DATA_TYPES[dt]
        wave, block, chunk = reduce_edges(g.plan_reduce_batch, es)
        lanes = [c for c in (16, 64) if c < wave]
        edges = lanes + [wave, block, 2 * chunk]
        cap = (1 << 19) // es
        size = draw_size(rng, i, cap, edges + [cap - 1])
        args, arrays = {"data_type": dt, "op": op}, {}
        if call == "run_batch_offsets_ptr":
            lens = draw_lengths(rng, size, edges)
            offsets, total = offsets_from(rng, lens)
            segments = list(zip(offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)))
            args.update(total=total, num_segments=int(lens.size))
            arrays["offsets"] = arr_in(offsets, draw_shift(rng, 4))
            nseg = lens.size
        else:
            count = max(1, min(size, int(rng.choice(edges + [1, 2, 5, 100, size // 2, size // 3])) + int(rng.integers(-1, 2)))) if size else 0
            nseg = min(size // count, 2000) if count else int(rng.integers(1, 4))
            total = count * nseg
            segments = [(p * count, (p + 1) * count) for p in range(nseg)]
            args.update(count=count, num_partitions=int(nseg))
        arrays["data"] = arr_in(draw_values(rng, dt, op, total, segments), draw_shift(rng, es))
        arrays["out"] = arr_out((nseg + 2) * comps, name, draw_shift(rng, es))
        out.append(new_step(unit, seed, i, call, "reduce:%d:%d" % (dt, op), args, arrays, total * es // 4, "dt%d" % dt, (call, op)))
        prev, prev_call = (dt, op), call
    return out


def reduce_segments(step):
    a = step["args"]
    if "offsets" in step["arrays"]:
        o = step["arrays"]["offsets"]["data"].astype(np.int64)
        return list(zip(o[:-1], o[1:]))
    return [(p * a["count"], (p + 1) * a["count"]) for p in range(a["num_partitions"])]


def exp_reduce(step, order="forward"):
    a = step["args"]
    name, comps = DATA_TYPES[a["data_type"]]
    rows = step["arrays"]["data"]["data"].reshape(-1, comps)
    out = step["arrays"]["out"]["data"].copy().reshape(-1, comps)
    for s, (b, e) in enumerate(reduce_segments(step)):
        out[s] = fold(rows[b:e], a["op"], order)
    return {"out": out.reshape(-1)}


def diag_reduce(step):
    g, es = G(), elem_bytes(step["args"]["data_type"])
    return batch_classes([e - b for b, e in reduce_segments(step)], lambda n: g.plan_reduce_batch(n, es)[0], 0)


def classes_reduce(step):
    g, es = G(), elem_bytes(step["args"]["data_type"])
    form = "offsets" if "offsets" in step["arrays"] else "equal"
    out = set()
    for b, e in reduce_segments(step):
        path, groups = g.plan_reduce_batch(int(e - b), es)
        if path:
            out.add("%s:%s" % (form, ("wave", "block", "long")[path - 1]))
            if path == 3 and groups >= 2:
                out.add(form + ":long:chunks>=2")
    return sorted(out)


def required_reduce():
    return ["offsets:wave", "offsets:block", "offsets:long", "offsets:long:chunks>=2", "equal:wave", "equal:block", "equal:long"]


# ---------------------------------------------------------------------------------------------------------------- BlellochScan


def gen_scan(g, rng, unit, seed, steps):
    dts = [int(x) for x in rng.permutation(12)[:3]]
    if len({elem_bytes(d) for d in dts}) < 2:
        dts[0] = 7 if elem_bytes(dts[1]) != 32 else 3
    out, prev, prev_call = [], None, None
    for i in range(steps):
        dt = draw_other(rng, dts, prev, i % 2 == 1)
        call = draw_other(rng, ["run_batch_offsets_ptr", "run_batch_offsets_ptr", "run_ptr"], prev_call, i % 3 == 0)
        es = elem_bytes(dt)
        name, comps = DATA_TYPES[dt]
        wave, block, chunk = reduce_edges(g.plan_scan_batch, es)
        lanes = [c for c in (128 // es, 512 // es) if 0 < c < wave]
        edges = lanes + [wave, block, 2 * chunk, 3 * chunk]
        cap = (1 << 19) // es
        size = draw_size(rng, i, cap, edges + [cap - 1])
        args, arrays = {"data_type": dt}, {}
        if call == "run_batch_offsets_ptr":
            lens = draw_lengths(rng, size, edges)
            offsets, total = offsets_from(rng, lens)
            args.update(total=total, num_segments=int(lens.size))
            arrays["offsets"] = arr_in(offsets, draw_shift(rng, 4))
        else:
            size = max(1, size)
            count = max(1, min(size, int(rng.choice(edges + [1, 2, 5, 100, size])) + int(rng.integers(-1, 2))))
            parts = min(max(1, size // count), 2000)
            total = count * parts
            args.update(count=count, num_partitions=int(parts))
        arrays["data"] = arr_inout(draw_values(rng, dt, SUM, total, ()), draw_shift(rng, es))
        out.append(new_step(unit, seed, i, call, "scan:%d" % dt, args, arrays, total * es // 4, "dt%d" % dt, (call,)))
        prev, prev_call = dt, call
    return out


def exp_scan(step, order="forward"):
    name, comps = DATA_TYPES[step["args"]["data_type"]]
    rows = step["arrays"]["data"]["data"].reshape(-1, comps)
    out = rows.copy()
    for b, e in reduce_segments(step):
        out[b:e] = exclusive_scan(rows[b:e], order)
    return {"data": out.reshape(-1)}


def diag_scan(step):
    if step["call"] != "run_batch_offsets_ptr":
        return {}
    g, es = G(), elem_bytes(step["args"]["data_type"])
    return batch_classes([e - b for b, e in reduce_segments(step)], lambda n: g.plan_scan_batch(n, es)[0], 0)


def classes_scan(step):
    g, es = G(), elem_bytes(step["args"]["data_type"])
    if step["call"] == "run_ptr":
        return ["run_ptr"]
    out = set()
    for b, e in reduce_segments(step):
        path, groups = g.plan_scan_batch(int(e - b), es)
        if path == 1:
            out.add("offsets:wave:%s" % ("128B" if (e - b) * es <= 128 else "512B" if (e - b) * es <= 512 else "2KiB"))
        elif path == 2:
            out.add("offsets:block")
        elif path == 3:
            out.add("offsets:long")
            if groups >= 3:
                out.add("offsets:long:chunks>=3")
    return sorted(out)


def required_scan():
    return ["offsets:wave:128B", "offsets:wave:512B", "offsets:wave:2KiB", "offsets:block", "offsets:long", "offsets:long:chunks>=3", "run_ptr"]


# ---------------------------------------------------------------------------------------------------------------- KeyRuns


def gen_key_runs(g, rng, unit, seed, steps):
    out, prev_bits, prev_variant = [], None, None
    cap = 1 << 17
    for i in range(steps):
        key_bits = draw_other(rng, (32, 64), prev_bits, i % 2 == 1)
        kt = "uint32" if key_bits == 32 else "uint64"
        call, unique, ranged = draw_other(rng, [(c, u, r) for c in ("run_ptr", "run_ptr", "reduce_by_key", "scan_by_key") for u in (True, False)
                                                for r in (True, False)], prev_variant, i % 3 == 0)
        tile = g.plan_key_runs(1, key_bits)[0]
        count = draw_size(rng, i, cap, [tile, 2 * tile, 16 * tile, cap - 1])
        begin_bit, end_bit = 0, key_bits
        if ranged:
            begin_bit = int(rng.integers(0, key_bits))
            end_bit = int(rng.integers(begin_bit, key_bits + 1))
        run_lens = draw_lengths(rng, count, [tile, 64, 4096 // (key_bits // 8)], most=int(rng.choice([3, 40, 3000])))
        run_lens = run_lens[run_lens > 0]
        if run_lens.sum() < count:
            run_lens = np.concatenate([run_lens, np.ones(count - int(run_lens.sum()), dtype=np.int64)])
        keys = np.repeat(draw_keys(rng, kt, run_lens.size), run_lens)
        assert keys.size == count
        mask = ((1 << end_bit) - 1) & ~((1 << begin_bit) - 1)
        heads = key_run_heads(keys, mask)
        R = heads.size
        max_runs = max(1, int(rng.choice([R - 1, R, R + 1, R // 2, R + 17, 1])))
        args = {"count": count, "key_bits": key_bits, "begin_bit": begin_bit, "end_bit": end_bit, "max_runs": max_runs, "true_runs": R}
        arrays = {"keys": arr_in(keys, draw_shift(rng, key_bits // 8)), "offsets": arr_out(max_runs + 1, np.uint32, draw_shift(rng, 4)),
                  "num_runs": arr_out(1, np.uint32, draw_shift(rng, 4))}
        if unique:
            arrays["unique_keys"] = arr_out(max_runs + 2, kt, draw_shift(rng, key_bits // 8))
        if call == "reduce_by_key":
            arrays["values"] = arr_in(rng.integers(0, 2 ** 32, count, dtype=np.uint32), draw_shift(rng, 4))
            arrays["out"] = arr_out(max_runs + 2, np.uint32, draw_shift(rng, 4))
        elif call == "scan_by_key":
            arrays["values"] = arr_inout(rng.integers(0, 2 ** 32, count, dtype=np.uint32), draw_shift(rng, 4))
        out.append(new_step(unit, seed, i, call, "runs", args, arrays, count, "bits%d" % key_bits, (call, unique, ranged)))
        prev_bits, prev_variant = key_bits, (call, unique, ranged)
    return out


def key_run_heads(keys, mask):
    if keys.size == 0:
        return np.zeros(0, dtype=np.int64)
    u = keys.view(uint_of(keys.dtype))
    diff = ((u[1:] ^ u[:-1]) & u.dtype.type(mask)) != 0
    return np.concatenate([[0], 1 + np.flatnonzero(diff)]).astype(np.int64)


def exp_key_runs(step):
    a, arrays = step["args"], step["arrays"]
    keys, count, max_runs = arrays["keys"]["data"], a["count"], a["max_runs"]
    mask = ((1 << a["end_bit"]) - 1) & ~((1 << a["begin_bit"]) - 1)
    heads = key_run_heads(keys, mask)
    shown = min(heads.size, max_runs)
    offsets = np.full(max_runs + 1, count, dtype=np.uint32)
    offsets[:shown] = heads[:shown]
    out = {"offsets": offsets, "num_runs": np.array([heads.size], dtype=np.uint32)}
    if "unique_keys" in arrays:
        uk = arrays["unique_keys"]["data"].copy()
        uk[:shown] = keys[heads[:shown]]
        out["unique_keys"] = uk
    o = offsets.astype(np.int64)
    if "values" in arrays:  # (uint32 sums wrap: sums in uint64, cut to 32 bits; the segments are the max_runs runs of the offsets)
        v = arrays["values"]["data"]
        before = np.concatenate([[0], np.cumsum(v, dtype=np.uint64)]).astype(np.uint64)
        if step["call"] == "reduce_by_key":
            res = arrays["out"]["data"].copy()
            res[:max_runs] = ((before[o[1:]] - before[o[:-1]]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out["out"] = res
        else:
            res = v.copy()
            b, e = int(o[0]), int(o[-1])
            res[b:e] = ((before[b:e] - np.repeat(before[o[:-1]], np.diff(o))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out["values"] = res
    return out


def classes_key_runs(step):
    a = step["args"]
    tiles = G().plan_key_runs(a["count"], a["key_bits"])[1]
    out = ["tiles:%s" % ("0" if tiles == 0 else "1" if tiles == 1 else "many"), "call:" + step["call"],
           "runs:%s" % ("below" if a["true_runs"] < a["max_runs"] else "at" if a["true_runs"] == a["max_runs"] else "above")]
    return out


def required_key_runs():
    return ["tiles:0", "tiles:1", "tiles:many", "call:run_ptr", "call:reduce_by_key", "call:scan_by_key", "runs:below", "runs:at", "runs:above"]


# ---------------------------------------------------------------------------------------------------------------- Select

STENCILS = {0: "float32", 1: "float64", 2: "int32", 3: "uint32", 12: "uint8"}
COMPARE = (np.equal, np.not_equal, np.less, np.less_equal, np.greater, np.greater_equal)


def gen_select(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    for i in range(steps):
        st = draw_other(rng, sorted(STENCILS), prev_type, i % 2 == 1)
        dt = np.dtype(STENCILS[st])
        variant = draw_other(rng, [(ix, ib, thr) for ix in (True, False) for ib in (0, 4, 8, 16, 32) for thr in (True, False)], prev_variant,
                             i % 3 == 0)
        with_indices, item_bytes, with_threshold = variant
        op = int(rng.integers(0, 6))
        tile = g.plan_select(1, st)[0]
        count = draw_size(rng, i, cap, [tile, 2 * tile, 8 * tile, cap - 1])
        if dt.kind == "f":
            threshold = float(rng.choice([0.0, 1.5, -2.0])) if with_threshold else None
            t = 0.0 if threshold is None else threshold
            pool = np.array([t, t, np.nextafter(dt.type(t), dt.type(np.inf)), np.nextafter(dt.type(t), dt.type(-np.inf)), -0.0, 0.0, np.nan, np.inf,
                             -np.inf, 7.0], dtype=dt)
        else:
            info = np.iinfo(dt)
            threshold = int(rng.choice([info.min, info.max, (info.min + info.max) // 2, 5])) if with_threshold else None
            t = 0 if threshold is None else threshold
            pool = np.array([t, t, min(t + 1, info.max), max(t - 1, info.min), info.min, info.max, 3, 0], dtype=dt)
        density = rng.choice([0, 1, 2, 2, 2])  # nothing but the threshold / nothing but one other value / the whole pool
        if density == 0:
            pool = pool[:1]
        elif density == 1:
            pool = pool[int(rng.integers(2, pool.size))][None]
        weights = rng.random(pool.size) ** 3
        stencil = pool[rng.choice(pool.size, count, p=weights / weights.sum())]
        with np.errstate(invalid="ignore"):
            S = int(COMPARE[op](stencil, dt.type(t)).sum())
        max_out = max(0, int(rng.choice([S, S, S + 5, S // 2, S - 1, count, 0])))
        args = {"count": count, "stencil_type": st, "op": op, "threshold": threshold, "item_bytes": item_bytes, "max_out": max_out, "selected": S}
        arrays = {"stencil": arr_in(stencil, draw_shift(rng, dt.itemsize)), "num_selected": arr_out(1, np.uint32, draw_shift(rng, 4))}
        if with_indices:
            arrays["out_indices"] = arr_out(max_out + 2, np.uint32, draw_shift(rng, 4))
        if item_bytes:
            arrays["items"] = arr_in(rng.integers(0, 256, count * item_bytes, dtype=np.uint8), draw_shift(rng, item_bytes))
            arrays["out_items"] = arr_out((max_out + 2) * item_bytes, np.uint8, draw_shift(rng, item_bytes))
        out.append(new_step(unit, seed, i, "run_ptr", "select", args, arrays, count, "stencil%d" % st, variant))
        prev_type, prev_variant = st, variant
    return out


def exp_select(step):
    a, arrays = step["args"], step["arrays"]
    stencil = arrays["stencil"]["data"]
    t = stencil.dtype.type(0 if a["threshold"] is None else a["threshold"])
    with np.errstate(invalid="ignore"):
        picked = np.flatnonzero(COMPARE[a["op"]](stencil, t))
    shown = picked[:a["max_out"]]
    out = {"num_selected": np.array([picked.size], dtype=np.uint32)}
    if "out_indices" in arrays:
        o = arrays["out_indices"]["data"].copy()
        o[:shown.size] = shown
        out["out_indices"] = o
    if "out_items" in arrays:
        ib = a["item_bytes"]
        o = arrays["out_items"]["data"].copy().reshape(-1, ib)
        o[:shown.size] = arrays["items"]["data"].reshape(-1, ib)[shown]
        out["out_items"] = o.reshape(-1)
    return out


def classes_select(step):
    a = step["args"]
    tiles = G().plan_select(a["count"], a["stencil_type"])[1]
    return ["tiles:%s" % ("0" if tiles == 0 else "1" if tiles == 1 else "many"),
            "room:%s" % ("short" if a["max_out"] < a["selected"] else "enough"),
            "density:%s" % ("none" if a["selected"] == 0 else "all" if a["selected"] == a["count"] else "some")]


def required_select():
    return ["tiles:0", "tiles:1", "tiles:many", "room:short", "room:enough", "density:none", "density:all", "density:some"]


# ---------------------------------------------------------------------------------------------------------------- SortedSearch

AUTO, DIRECT, INDEXED = range(3)


def fanout(key_type):
    return 128 // np.dtype(key_type).itemsize


def gen_sorted_search(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 16
    built = None  # (step index that holds the haystack, key type, hay count, TOP_ENTRIES) of the index the object remembers
    for i in range(steps):
        reuse = built is not None and rng.random() < 0.35
        if reuse:
            _, key_type, hay_count, top = built
            hay = out[-1]["arrays"]["hay"]
            path = out[-1]["args"]["path_option"] if out[-1]["args"]["path_option"] != DIRECT else AUTO
            variant = (path, top == fanout(key_type), draw_other(rng, ("lower", "upper", "both"), None, False), "reuse")
        else:
            key_type = draw_other(rng, KEY_TYPES, prev_type, i % 2 == 1)
            F = fanout(key_type)
            variant = draw_other(rng, [(p, t, o, c) for p in (AUTO, DIRECT, INDEXED) for t in (True, False) for o in ("lower", "upper", "both")
                                       for c in ("run", "run", "index")], prev_variant, i % 3 == 0)
            if variant[3] == "index" and variant[0] == DIRECT:
                variant = (INDEXED,) + variant[1:]
            path, top = variant[0], F if variant[1] else (8192 if F == 32 else 4096)
            hay_count = draw_size(rng, i, cap, [F, F * F, F ** 3, top, top * F, cap - 1])
            hay = arr_in(in_sort_order(draw_keys(rng, key_type, hay_count)), draw_shift(rng, np.dtype(key_type).itemsize))
        kb = np.dtype(key_type).itemsize
        options = [("search", "PATH", path), ("search", "TOP_ENTRIES", top)]
        levels = g.plan_sorted_search(hay_count, 1, key_type, top)[1]
        args = {"key_type": key_type, "hay_count": hay_count, "path_option": path, "top_entries": top, "levels": levels, "reuse_index": reuse}
        arrays = {"hay": dict(hay, carry=True) if reuse else hay}
        if variant[3] == "index":
            call, needle_count = "index_ptr", 0
        else:
            call = "run_ptr"
            needle_count = int(rng.choice([1, 2, 65, int(2.0 ** rng.uniform(0, 14)), max(1, hay_count // 128), max(1, hay_count // 128 - 1)]))
            pool = hay["data"] if hay_count and rng.random() < 0.7 else draw_keys(rng, key_type, 8)
            needles = np.concatenate([pool[rng.integers(0, pool.size, needle_count)], draw_keys(rng, key_type, needle_count)])
            needles = needles[rng.permutation(needles.size)[:needle_count]]
            args.update(needle_count=needle_count, outputs=variant[2])
            arrays["needles"] = arr_in(needles, draw_shift(rng, kb))
            if variant[2] in ("lower", "both"):
                arrays["out_lower"] = arr_out(needle_count, np.uint32, draw_shift(rng, 4))
            if variant[2] in ("upper", "both"):
                arrays["out_upper"] = arr_out(needle_count, np.uint32, draw_shift(rng, 4))
        taken = diag_sorted_search_of(g, args, call, needle_count)["last"]
        if not reuse:  # (a call that built no index leaves nothing this module relies on)
            built = (i, key_type, hay_count, top) if taken[0] == INDEXED and taken[2] == (1 if call == "index_ptr" else 2) else None
        out.append(new_step(unit, seed, i, call, "search", args, arrays, hay_count, key_type, variant, options))
        prev_type, prev_variant = key_type, variant
    return out


def diag_sorted_search_of(g, a, call, needle_count):
    auto, levels, _, _ = g.plan_sorted_search(a["hay_count"], needle_count, a["key_type"], a["top_entries"])
    if call == "index_ptr":
        return {"last": (INDEXED, levels, 1) if levels else (DIRECT, 0, 0)}
    path, reuse = a["path_option"], a["reuse_index"]
    taken = DIRECT if levels == 0 or path == DIRECT else INDEXED if path == INDEXED or reuse else auto
    search = 1 if needle_count else 0
    if taken == DIRECT:
        return {"last": (DIRECT, 0, search)}
    return {"last": (INDEXED, levels, search + (0 if reuse else 1))}


def diag_sorted_search(step):
    if step["call"] == "index_ptr" and step["args"]["levels"] == 0:
        return {}  # (what an index call without a level reports is not stated in the header)
    return diag_sorted_search_of(G(), step["args"], step["call"], step["args"].get("needle_count", 0))


def exp_sorted_search(step):
    arrays = step["arrays"]
    if step["call"] == "index_ptr":
        return {}
    hay, needles = key_code(arrays["hay"]["data"], False), key_code(arrays["needles"]["data"], False)
    out = {}
    if "out_lower" in arrays:
        out["out_lower"] = np.searchsorted(hay, needles, "left").astype(np.uint32)
    if "out_upper" in arrays:
        out["out_upper"] = np.searchsorted(hay, needles, "right").astype(np.uint32)
    return out


def classes_sorted_search(step):
    a = step["args"]
    last = diag_sorted_search_of(G(), a, step["call"], a.get("needle_count", 0))["last"]
    out = ["direct" if last[0] == DIRECT else "indexed:%d" % last[1]]
    if a["reuse_index"]:
        out.append("reuse")
    if step["call"] == "index_ptr":
        out.append("index_ptr")
    return out


def required_sorted_search():
    return ["direct", "indexed:1", "indexed:2", "indexed:3", "reuse", "index_ptr"]


# ---------------------------------------------------------------------------------------------------------------- Merge and SetOps


def draw_two_sorted(rng, key_type, size):
    """(a, b): two arrays sorted in the sort's order out of ONE pool of keys (heavy ties across them), one side empty now and then."""
    side = int(rng.integers(0, 6))
    a_count = 0 if side == 0 else size if side == 1 else int(rng.integers(0, size + 1))
    both = draw_keys(rng, key_type, size)
    return in_sort_order(both[:a_count]), in_sort_order(both[a_count:])


def gen_merge(g, rng, unit, seed, steps, set_ops=False):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    for i in range(steps):
        key_type = draw_other(rng, KEY_TYPES, prev_type, i % 2 == 1)
        kb = np.dtype(key_type).itemsize
        if set_ops:
            variant = draw_other(rng, [(v, o, m) for v in (True, False) for o in ("union", "intersection", "difference", "symmetric_difference")
                                       for m in ("count_only", "short", "short", "exact", "room", "room")], prev_variant, i % 3 == 0)
        else:
            variant = draw_other(rng, [(True,), (False,)], prev_variant, i % 3 == 0)
        with_vals = variant[0]
        tile = g.plan_merge(1, 1, key_type, with_vals)[0]
        size = draw_size(rng, i, cap, [tile, 2 * tile, 8 * tile, cap - 1])
        a, b = draw_two_sorted(rng, key_type, size)
        if set_ops:
            S = set_ops_kept(a, b, variant[1]).size
            mode = variant[2]
            max_out = {"count_only": 0, "short": int(rng.choice([S // 2, max(0, S - 1)])), "exact": S, "room": S + int(rng.integers(1, 9))}[mode]
            if max_out == 0:  # (a call with max_out 0 only counts, and takes no values)
                mode = "count_only"
            with_vals = with_vals and mode != "count_only"
        args = {"key_type": key_type, "a_count": int(a.size), "b_count": int(b.size), "with_vals": with_vals}
        arrays = {"a_keys": arr_in(a, draw_shift(rng, kb)), "b_keys": arr_in(b, draw_shift(rng, kb))}
        if with_vals:
            arrays["a_vals"] = arr_in(rng.integers(0, 2 ** 32, a.size, dtype=np.uint32), draw_shift(rng, 4))
            arrays["b_vals"] = arr_in(rng.integers(0, 2 ** 32, b.size, dtype=np.uint32), draw_shift(rng, 4))
        if set_ops:
            args.update(op=variant[1], max_out=max_out, kept=S, count_only=mode == "count_only")
            arrays["num_out"] = arr_out(1, np.uint32, draw_shift(rng, 4))
            room = max_out + 3
            call = "run_ptr"
        else:
            room, mode, call = size, "exact", "run_ptr"
        if mode != "count_only":
            arrays["out_keys"] = arr_out(room, key_type, draw_shift(rng, kb))
            if with_vals:
                arrays["out_vals"] = arr_out(room, np.uint32, draw_shift(rng, 4))
        out.append(new_step(unit, seed, i, call, "set_ops" if set_ops else "merge", args, arrays, size, key_type, variant))
        prev_type, prev_variant = key_type, variant
    return out


def gen_set_ops(g, rng, unit, seed, steps):
    return gen_merge(g, rng, unit, seed, steps, set_ops=True)


def merge_order(a, b):
    return np.argsort(np.concatenate([key_code(a, False), key_code(b, False)]), kind="stable")


def exp_merge(step):
    arrays = step["arrays"]
    a, b = arrays["a_keys"]["data"], arrays["b_keys"]["data"]
    order = merge_order(a, b)
    out = {"out_keys": np.concatenate([a, b])[order]}
    if "out_vals" in arrays:
        out["out_vals"] = np.concatenate([arrays["a_vals"]["data"], arrays["b_vals"]["data"]])[order]
    return out


def set_ops_kept(a, b, op):
    """Indices into A || B of the kept elements, in merge's order: the rank rule of the header."""
    ca, cb = key_code(a, False), key_code(b, False)
    match_a = (np.arange(a.size) - np.searchsorted(ca, ca, "left")) < (np.searchsorted(cb, ca, "right") - np.searchsorted(cb, ca, "left"))
    match_b = (np.arange(b.size) - np.searchsorted(cb, cb, "left")) < (np.searchsorted(ca, cb, "right") - np.searchsorted(ca, cb, "left"))
    none_b = np.zeros(b.size, dtype=bool)
    keep_a, keep_b = {"union": (np.ones(a.size, dtype=bool), ~match_b), "intersection": (match_a, none_b), "difference": (~match_a, none_b),
                      "symmetric_difference": (~match_a, ~match_b)}[op]
    order = np.argsort(np.concatenate([ca, cb]), kind="stable")
    return order[np.concatenate([keep_a, keep_b])[order]]


def exp_set_ops(step):
    a_, arrays = step["args"], step["arrays"]
    a, b = arrays["a_keys"]["data"], arrays["b_keys"]["data"]
    kept = set_ops_kept(a, b, a_["op"])
    out = {"num_out": np.array([kept.size], dtype=np.uint32)}
    shown = kept[:a_["max_out"]]
    if "out_keys" in arrays:
        o = arrays["out_keys"]["data"].copy()
        o[:shown.size] = np.concatenate([a, b])[shown]
        out["out_keys"] = o
    if "out_vals" in arrays:
        o = arrays["out_vals"]["data"].copy()
        o[:shown.size] = np.concatenate([arrays["a_vals"]["data"], arrays["b_vals"]["data"]])[shown]
        out["out_vals"] = o
    return out


def diag_merge(step):
    a = step["args"]
    return {"last": G().plan_merge(a["a_count"], a["b_count"], a["key_type"], a["with_vals"])[1:3]}


def diag_set_ops(step):
    a = step["args"]
    return {"last": G().plan_set_ops(a["a_count"], a["b_count"], a["key_type"], "out_keys" in step["arrays"] and a["max_out"] > 0)[1:3]}


def classes_merge(step):
    a = step["args"]
    tiles = diag_merge(step)["last"][0]
    out = ["tiles:%s" % ("0" if tiles == 0 else "1" if tiles == 1 else "many")]
    if a["a_count"] + a["b_count"] and not (a["a_count"] and a["b_count"]):
        out.append("one_sided")
    return out


def required_merge():
    return ["tiles:0", "tiles:1", "tiles:many", "one_sided"]


def classes_set_ops(step):
    a = step["args"]
    tiles, kernels = diag_set_ops(step)["last"]
    return ["tiles:%s" % ("0" if tiles == 0 else "1" if tiles == 1 else "many"), "kernels:%d" % kernels, "op:" + a["op"],
            "room:%s" % ("count_only" if a["count_only"] else "short" if a["max_out"] < a["kept"] else "enough")]


def required_set_ops():
    return ["tiles:0", "tiles:1", "tiles:many", "kernels:1", "kernels:3", "kernels:4", "op:union", "op:intersection", "op:difference",
            "op:symmetric_difference", "room:count_only", "room:short", "room:enough"]


# ---------------------------------------------------------------------------------------------------------------- Histogram

LDS, GLOBAL = 0, 1


def gen_histogram(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    carried = None  # (bins, the counts the last step left) for a step that accumulates into the same device array
    for i in range(steps):
        variant = draw_other(rng, [(m, acc) for m in ("even", "even", "edges") for acc in ("no", "fresh", "carry")], prev_variant, i % 3 == 0)
        mode, acc = variant
        key_type = draw_other(rng, KEY_TYPES if mode == "edges" else ("uint32", "int32", "float32", "float64"), prev_type, i % 2 == 1)
        dt = np.dtype(key_type)
        if acc == "carry" and carried is not None:
            bins = carried[0]
            if bins > 8192:
                mode, variant = "even", ("even", acc)
                if key_type in ("uint64", "int64"):
                    key_type, dt = "uint32", np.dtype("uint32")
        else:
            bins = int(rng.choice([1, 2, 7, 256, int(2.0 ** rng.uniform(0, 13)), 8191, 8192] + ([8193, 20000, 20000] if mode == "even" else [])))
            if acc == "carry":
                acc, variant = "fresh", (mode, "fresh")
        tile = g.plan_histogram(1, bins, key_type, mode)[2]
        count = draw_size(rng, i, cap, [tile, 2 * tile, 8 * tile, cap - 1])
        args = {"key_type": key_type, "count": count, "bins": bins, "accumulate": acc != "no", "mode": mode}
        arrays = {}
        if mode == "even":
            if dt.kind == "f":
                lo = float(dt.type(rng.choice([-1000.5, 0.0, 0.1, 3.0])))
                hi = float(dt.type(lo + float(rng.choice([1.0, 0.3, 1e6]))))
                x = (lo + (hi - lo) * rng.uniform(-0.2, 1.2, count)).astype(dt)
                special = np.array([lo, hi, np.nan, -0.0, np.inf, -np.inf, np.nextafter(dt.type(hi), dt.type(-np.inf))], dtype=dt)
            else:
                info = np.iinfo(dt)
                width = int(rng.choice([1, 3, 1000, (int(info.max) - int(info.min)) // bins]))
                width = max(1, min(width, (int(info.max) - int(info.min)) // bins))
                lo = int(rng.integers(info.min, int(info.max) - width * bins + 1))
                hi = lo + width * bins
                a, b = max(int(info.min), lo - width * bins // 4 - 2), min(int(info.max), hi + width * bins // 4 + 2)
                x = rng.integers(a, b + 1, count, dtype=np.int64 if dt.kind == "i" else np.uint64).astype(dt)
                special = np.array([lo, hi - 1, min(hi, info.max), max(lo - 1, info.min), info.min, info.max], dtype=dt)
            args.update(lo=lo, hi=hi)
        else:
            pool = draw_keys(rng, key_type, bins + 1 + 8)
            if dt.kind == "f":
                pool = pool[~np.isnan(pool)]
                pool = np.concatenate([pool, rng.standard_normal(bins + 9).astype(dt)])[:bins + 9]
            edges = np.sort(pool)[rng.integers(0, 2):][:bins + 1]
            if edges.size < bins + 1:
                edges = np.sort(np.concatenate([edges, np.repeat(edges[-1:], bins + 1 - edges.size)]))
            x = np.concatenate([edges[rng.integers(0, edges.size, count)], draw_keys(rng, key_type, count)])[rng.permutation(2 * count)[:count]]
            special = edges[[0, -1]]
            arrays["edges"] = arr_in(edges, draw_shift(rng, dt.itemsize))
        if count:
            at = rng.integers(0, count, min(count, 12))
            x[at] = special[rng.integers(0, special.size, at.size)]
        if rng.random() < 0.2 and count:  # one value: the held-back add of a wave
            x[:] = x[0]
        arrays["samples"] = arr_in(x, draw_shift(rng, dt.itemsize))
        if acc == "carry" and carried is not None:
            arrays["counts"] = arr_inout(carried[1], carried[2], carry=True)
        elif acc == "fresh":
            prior = rng.integers(0, 2 ** 32, bins, dtype=np.uint32)
            prior[::3] = np.uint32(0xFFFFFFFF) - rng.integers(0, 3, prior[::3].size, dtype=np.uint32)
            arrays["counts"] = arr_inout(prior, draw_shift(rng, 4))
        else:
            arrays["counts"] = arr_out(bins, np.uint32, draw_shift(rng, 4))
        step = new_step(unit, seed, i, "run_%s_ptr" % mode, "histogram", args, arrays, count, key_type, variant)
        out.append(step)
        carried = (bins, exp_histogram(step)["counts"], arrays["counts"]["shift"])
        prev_type, prev_variant = key_type, variant
    return out


def exp_histogram(step):
    a, arrays = step["args"], step["arrays"]
    x, bins = arrays["samples"]["data"], a["bins"]
    if a["mode"] == "even":
        if x.dtype.kind == "f":
            d = x.astype(np.float64)
            lo, hi = float(x.dtype.type(a["lo"])), float(x.dtype.type(a["hi"]))
            scale = float(bins) / (hi - lo)
            with np.errstate(invalid="ignore"):
                inside = (d >= lo) & (d < hi)
            at = np.minimum(((d[inside] - lo) * scale).astype(np.uint32), np.uint32(bins - 1)).astype(np.int64)
        else:
            v = x.astype(np.int64)
            inside = (v >= a["lo"]) & (v < a["hi"])
            at = ((v[inside] - a["lo"]) // ((a["hi"] - a["lo"]) // bins)).astype(np.int64)
    else:
        edges = arrays["edges"]["data"]
        at = np.searchsorted(edges, x, side="right").astype(np.int64) - 1
        ok = (at >= 0) & (at < bins)
        if x.dtype.kind == "f":
            ok &= ~np.isnan(x)
        at = at[ok]
    counts = np.bincount(at, minlength=bins).astype(np.uint64)
    if a["accumulate"]:
        counts = counts + arrays["counts"]["data"].astype(np.uint64)
    return {"counts": (counts & np.uint64(0xFFFFFFFF)).astype(np.uint32)}


def diag_histogram(step):
    a = step["args"]
    path, _, _, groups, kernels, _ = G().plan_histogram(a["count"], a["bins"], a["key_type"], a["mode"])
    if a["accumulate"] and (path == GLOBAL or a["count"] == 0):
        kernels -= 1
    return {"last": (path, groups, kernels)}


def classes_histogram(step):
    a = step["args"]
    path, groups, _ = diag_histogram(step)["last"]
    return ["%s:%s" % (a["mode"], "lds" if path == LDS else "atomics"), "%s:%s" % ("lds" if path == LDS else "atomics", step["variant"][1]),
            "groups:%s" % ("0" if groups == 0 else "1" if groups == 1 else "many")]


def required_histogram():
    return ["even:lds", "even:atomics", "edges:lds", "lds:no", "lds:fresh", "lds:carry", "atomics:no", "atomics:fresh", "atomics:carry", "groups:0",
            "groups:1", "groups:many"]


# ---------------------------------------------------------------------------------------------------------------- Expand


def gen_expand(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    subsets = [(s, r, t) for s in (True, False) for r in (True, False) for t in (True, False)]
    for i in range(steps):
        item_bytes = draw_other(rng, (4, 8, 16, 32), prev_type, i % 2 == 1)
        variant = draw_other(rng, subsets, prev_variant, i % 3 == 0)
        tile = g.plan_expand(1, 1)[0]
        size = draw_size(rng, i, cap, [tile, 2 * tile, 8 * tile, cap - 1])
        lens = draw_lengths(rng, size, [tile, 64], most=int(rng.choice([3, 50, 400])))
        if rng.random() < 0.5:  # many empty segments between the others
            lens = np.concatenate([lens, np.zeros(int(rng.choice([10, 1000, 3 * tile])), dtype=np.int64)])
            rng.shuffle(lens)
        if i % 7 == 6:
            lens = lens[:0]
        offsets, _ = offsets_from(rng, lens)
        total = max(0, int(offsets[-1]) + int(rng.choice([0, 0, 3, -1, -(int(offsets[-1]) // 3)])))  # the cover partial, exact, or cut short
        nseg = int(lens.size)
        args = {"num_segments": nseg, "total": total, "item_bytes": item_bytes, "end": int(offsets[-1])}
        arrays = {"offsets": arr_in(offsets, draw_shift(rng, 4))}
        if variant[0]:
            arrays["out_segments"] = arr_out(total, np.uint32, draw_shift(rng, 4))
        if variant[1]:
            arrays["out_ranks"] = arr_out(total, np.uint32, draw_shift(rng, 4))
        if variant[2]:
            arrays["items"] = arr_in(rng.integers(0, 256, nseg * item_bytes, dtype=np.uint8), draw_shift(rng, item_bytes))
            arrays["out_items"] = arr_out(total * item_bytes, np.uint8, draw_shift(rng, item_bytes))
        out.append(new_step(unit, seed, i, "run_ptr", "expand", args, arrays, total, "items%d" % item_bytes, variant))
        prev_type, prev_variant = item_bytes, variant
    return out


def exp_expand(step):
    a, arrays = step["args"], step["arrays"]
    offsets, total, nseg = arrays["offsets"]["data"].astype(np.int64), a["total"], a["num_segments"]
    j = np.arange(total)
    seg = np.searchsorted(offsets, j, side="right") - 1
    covered = (seg >= 0) & (seg < nseg)
    at = seg[covered]
    out = {}
    if "out_segments" in arrays:
        o = arrays["out_segments"]["data"].copy()
        o[covered] = at
        out["out_segments"] = o
    if "out_ranks" in arrays:
        o = arrays["out_ranks"]["data"].copy()
        o[covered] = j[covered] - offsets[at]
        out["out_ranks"] = o
    if "out_items" in arrays:
        ib = a["item_bytes"]
        o = arrays["out_items"]["data"].copy().reshape(-1, ib)
        o[covered] = arrays["items"]["data"].reshape(-1, ib)[at]
        out["out_items"] = o.reshape(-1)
    return out


def diag_expand(step):
    a = step["args"]
    outputs = any(n in step["arrays"] for n in ("out_segments", "out_ranks", "out_items"))
    return {"last": G().plan_expand(a["total"], a["num_segments"])[1:3] if outputs and a["total"] and a["num_segments"] else (0, 0)}


def classes_expand(step):
    a = step["args"]
    tiles = diag_expand(step)["last"][0]
    return ["tiles:%s" % ("0" if tiles == 0 else "1" if tiles == 1 else "many"),
            "cover:%s" % ("short" if a["total"] < a["end"] else "exact" if a["total"] == a["end"] else "partial")]


def required_expand():
    return ["tiles:0", "tiles:1", "tiles:many", "cover:short", "cover:exact", "cover:partial"]


# ---------------------------------------------------------------------------------------------------------------- Gather


def gen_gather(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 16
    for i in range(steps):
        ib = draw_other(rng, (4, 8, 16, 32), prev_type, i % 2 == 1)
        call = draw_other(rng, ("run_ptr", "run_batch_ptr", "run_batch_offsets_ptr", "scatter_ptr"), prev_variant, i % 3 == 0)
        tile = g.plan_gather(1, ib)[0]
        size = draw_size(rng, i, cap, [tile, 2 * tile, 8 * tile, cap - 1])
        args, arrays = {"item_bytes": ib}, {}
        bad = float(rng.choice([0.0, 0.05, 0.5]))  # the share of indices that are out of range

        def spoil(idx, limit):
            idx = idx.astype(np.uint32)
            where = rng.random(idx.size) < bad
            idx[where] = rng.choice(np.array([limit, limit + 1, 0xFFFFFFFF, 0x80000000], dtype=np.uint64), int(where.sum())).astype(np.uint32)
            return idx

        if call == "run_ptr":
            item_count = int(rng.choice([1, 2, 1000, size + 1, cap]))
            idx = spoil(rng.integers(0, item_count, size), item_count)
            args.update(item_count=item_count, count=size)
            entries, out_entries = size, size
        elif call == "scatter_ptr":
            out_count = size + int(rng.integers(0, 100))
            count = int(rng.integers(0, out_count + 1))
            idx = spoil(rng.permutation(out_count)[:count], out_count)
            args.update(count=count, out_count=out_count)
            item_count, entries, out_entries = count, count, out_count
        else:
            k = int(rng.choice([1, 2, 7, 64, 513]))
            if call == "run_batch_ptr":
                count = max(1, int(rng.choice([1, 5, 100, 5000, max(1, size)])))
                count = min(count, max(1, size))
                parts = size // count
                lens = np.full(parts, count, dtype=np.int64)
                total = count * parts
                args.update(count=count, num_partitions=int(parts), k=k)
            else:
                lens = draw_lengths(rng, size, [k, 64, tile])
                offsets, total = offsets_from(rng, lens)
                args.update(total=total, num_segments=int(lens.size), k=k)
                arrays["offsets"] = arr_in(offsets, draw_shift(rng, 4))
            rows = lens.size
            idx = spoil(rng.integers(0, np.maximum(1, np.repeat(lens, k))), 0)
            if bad:  # an index at or just behind the end of its own segment
                where = rng.random(idx.size) < 0.1
                idx[where] = np.repeat(lens, k)[where] + rng.integers(0, 2, int(where.sum()))
            item_count, entries, out_entries = total, rows * k, rows * k
        arrays["items"] = arr_in(rng.integers(0, 256, item_count * ib, dtype=np.uint8), draw_shift(rng, ib))
        arrays["indices"] = arr_in(idx, draw_shift(rng, 4))
        arrays["out"] = arr_out(out_entries * ib, np.uint8, draw_shift(rng, ib))
        args["entries"] = int(entries)
        out.append(new_step(unit, seed, i, call, "gather", args, arrays, size, "items%d" % ib, (call,)))
        prev_type, prev_variant = ib, call
    return out


def exp_gather(step):
    a, arrays = step["args"], step["arrays"]
    ib = a["item_bytes"]
    items, idx = arrays["items"]["data"].reshape(-1, ib), arrays["indices"]["data"].astype(np.int64)
    out = arrays["out"]["data"].copy().reshape(-1, ib)
    if step["call"] == "run_ptr":
        ok = idx < a["item_count"]
        out[np.flatnonzero(ok)] = items[idx[ok]]
    elif step["call"] == "scatter_ptr":
        ok = idx < a["out_count"]
        out[idx[ok]] = items[np.flatnonzero(ok)]
    else:
        k = a["k"]
        if step["call"] == "run_batch_ptr":
            begin = np.arange(a["num_partitions"], dtype=np.int64) * a["count"]
            lens = np.full(a["num_partitions"], a["count"], dtype=np.int64)
        else:
            o = arrays["offsets"]["data"].astype(np.int64)
            begin, lens = o[:-1], np.diff(o)
        j = np.tile(np.arange(k), lens.size)
        row_len, row_begin = np.repeat(lens, k), np.repeat(begin, k)
        ok = (j < np.minimum(k, row_len)) & (idx < row_len)
        out[np.flatnonzero(ok)] = items[row_begin[ok] + idx[ok]]
    return {"out": out.reshape(-1)}


def diag_gather(step):
    a = step["args"]
    if not gather_work(step):
        return {"last": (0, 0)}
    ib = a["item_bytes"]
    piece = min(ib, 16)
    side = step["arrays"]["items" if step["call"] == "scatter_ptr" else "out"]
    lo = (side["shift"] % 16) // piece
    tile = G().plan_gather(1, ib)[0]
    return {"last": (-(-(lo + a["entries"] * (ib // piece)) // (tile * (ib // piece))), 1)}


def gather_work(step):
    a = step["args"]
    if not a["entries"]:
        return False
    if step["call"] == "run_ptr":
        return a["item_count"] > 0
    if step["call"] == "scatter_ptr":
        return a["out_count"] > 0
    return (a["total"] if "total" in a else a["count"] * a["num_partitions"]) > 0


def classes_gather(step):
    tiles = diag_gather(step)["last"][0]
    return ["%s:tiles:%s" % (step["call"], "0" if tiles == 0 else "1" if tiles == 1 else "many")]


def required_gather():
    return ["%s:tiles:%s" % (c, t) for c in ("run_ptr", "run_batch_ptr", "run_batch_offsets_ptr", "scatter_ptr") for t in ("1", "many")]


# ---------------------------------------------------------------------------------------------------------------- TopK

CANDIDATES, FULL = 1, 2
WAVE, BLOCK, LONG, LOOP, BINNED = 1, 2, 3, 4, 5


def gen_top_k(g, rng, unit, seed, steps):
    out, prev_type, prev_variant = [], None, None
    cap = 1 << 17
    for i in range(steps):
        key_type = draw_other(rng, KEY_TYPES, prev_type, i % 2 == 1)
        kb = np.dtype(key_type).itemsize
        variant = draw_other(rng, [(o, p, c, l) for o in ((1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1), (0, 0, 1), (1, 0, 1)) for p in (0, 1, 2)
                                   for c in (256, 0) for l in (0, 3000)], prev_variant, i % 3 == 0)
        outputs, path, cand, loop_min = variant
        call = str(rng.choice(["run_ptr", "run_batch_ptr", "run_batch_offsets_ptr"]))
        if i % 10 == 1:  # a large step of equal partitions beyond the workgroup tiles: the streaming kernel, or the loop
            call = "run_batch_ptr"
        largest, sorted_ = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        limits = g.plan_top_k_batch(1, 1, 1, key_type)["limits"]
        sort_limit = last_where(lambda c: g.plan_batch(c, kb, True)[0] <= 2)
        tile = g.plan_top_k(1, 1, key_type)["tile"]
        size = draw_size(rng, i, cap, limits + [tile, 2 * tile, 3000, cap - 1])
        args = {"key_type": key_type, "largest": largest, "sorted": sorted_, "path_option": path, "cand_capacity": cand, "loop_min": loop_min,
                "outputs": outputs}
        arrays = {}
        if call == "run_ptr":
            count = size
            k = min(count, int(rng.choice([0, 1, 2, 100, count // 2, max(0, count - 1), count, sort_limit + 1])))
            args.update(count=count, k=k)
            total, rows = count, 1
        elif call == "run_batch_ptr":
            count = max(1, min(max(1, size), int(rng.choice(limits + [1, 2, 100, 3000, size, size // 2, size // 3])) + int(rng.integers(-1, 2))))
            if i % 10 == 1:
                count = max(1, size // int(rng.integers(2, 4)))
            parts = min(max(1, size) // count, 300)
            k = max(1, min(count, int(rng.choice([1, 2, 64, count // 2 + 1, count, sort_limit + 1]))))
            args.update(count=count, num_partitions=int(parts), k=k)
            total, rows = count * parts, parts
        else:
            lens = draw_lengths(rng, size, limits, most=60)
            offsets, total = offsets_from(rng, lens)
            k = max(1, int(rng.choice([1, 2, 64, 513, int(lens.max()) + 1, sort_limit + 1])))
            if lens.size * k > 1 << 20:
                k = 64
            args.update(total=total, num_segments=int(lens.size), k=k)
            arrays["offsets"] = arr_in(offsets, draw_shift(rng, 4))
            rows = int(lens.size)
        keys = draw_keys(rng, key_type, total)
        if rng.random() < 0.3 and total:  # keys crowded into one bucket of the top digit: the candidates do not fit a small capacity
            u = uint_of(key_type)
            keys = ((keys.view(u) & u.type((1 << (8 * kb - 12)) - 1)) | (keys.view(u)[0] & ~u.type((1 << (8 * kb - 12)) - 1))).view(keys.dtype)
        arrays["keys"] = arr_in(keys, draw_shift(rng, kb))
        if outputs[0]:
            arrays["out_keys"] = arr_out(rows * k + 3, key_type, draw_shift(rng, kb))
        if outputs[1]:
            arrays["out_indices"] = arr_out(rows * k + 3, np.uint32, draw_shift(rng, 4))
        if outputs[2]:
            arrays["out_kth"] = arr_out(rows + 2, key_type, draw_shift(rng, kb))
        options = [("top_k", "PATH", path), ("top_k", "CAND_CAPACITY", cand), ("top_k", "BATCH_LOOP_MIN", loop_min)]
        out.append(new_step(unit, seed, i, call, "top_k", args, arrays, total, key_type, variant, options))
        prev_type, prev_variant = key_type, variant
    return out


def top_k_segments(step):
    a = step["args"]
    if step["call"] == "run_ptr":
        return [(0, a["count"])]
    if step["call"] == "run_batch_ptr":
        return [(p * a["count"], (p + 1) * a["count"]) for p in range(a["num_partitions"])]
    o = step["arrays"]["offsets"]["data"].astype(np.int64)
    return list(zip(o[:-1], o[1:]))


def exp_top_k(step):
    a, arrays = step["args"], step["arrays"]
    keys, k = arrays["keys"]["data"], a["k"]
    out = {n: arrays[n]["data"].copy() for n in ("out_keys", "out_indices", "out_kth") if n in arrays}
    for s, (b, e) in enumerate(top_k_segments(step)):
        ks = min(k, e - b)
        if ks <= 0:
            continue
        head = np.argsort(key_code(keys[b:e], a["largest"]), kind="stable")[:ks]
        if "out_kth" in out:
            out["out_kth"][s] = keys[b + head[-1]]
        if not a["sorted"]:
            head = np.sort(head)
        if "out_keys" in out:
            out["out_keys"][s * k:s * k + ks] = keys[b + head]
        if "out_indices" in out:
            out["out_indices"][s * k:s * k + ks] = head
    return out


def diag_top_k(step):
    g, a = G(), step["args"]
    arrays = bool(a["outputs"][0] or a["outputs"][1])
    if step["call"] == "run_ptr":
        if not a["k"]:
            return {"path": 0, "candidates": 0, "ties": 0, "kernels": 0}
        plan = g.plan_top_k(a["count"], a["k"], a["key_type"], a["sorted"], arrays, a["path_option"], a["cand_capacity"])
        code = key_code(step["arrays"]["keys"]["data"], a["largest"])
        kth = np.partition(code, a["k"] - 1)[a["k"] - 1]
        shift = plan["digits"][0][0]
        bucket = int(((code >> code.dtype.type(shift)) == (kth >> code.dtype.type(shift))).sum())
        fits = a["path_option"] != FULL and bucket <= plan["capacity"]
        return {"path": CANDIDATES if fits else FULL, "candidates": bucket if fits else 0, "ties": a["k"] - int((code < kth).sum()),
                "kernels": plan["kernels"]}
    offsets_form = step["call"] == "run_batch_offsets_ptr"
    plan = g.plan_top_k_batch(a["total"] if offsets_form else a["count"], a["num_segments"] if offsets_form else a["num_partitions"], a["k"],
                              a["key_type"], offsets_form, a["sorted"], arrays, a["loop_min"])
    out = {"kernels": plan["kernels"]}
    limits = plan["limits"]
    lens = [e - b for b, e in top_k_segments(step)]
    if plan["path"] == LOOP:  # (the single call under the object's options, which the batch's plan is not told, once per partition)
        single = g.plan_top_k(a["count"], a["k"], a["key_type"], a["sorted"], arrays, a["path_option"], a["cand_capacity"])
        out.update(wave=0, block=0, long=len(lens), kernels=len(lens) * single["kernels"])
    elif plan["path"] != 0:
        out.update(batch_classes(lens, lambda n: 1 if n <= limits[0] else 2 if n <= limits[3] else 3, 0))
    return out


def classes_top_k(step):
    g, a = G(), step["args"]
    d = diag_top_k(step)
    if step["call"] == "run_ptr":
        return [] if not a["k"] else ["single:%s" % ("candidates" if d["path"] == CANDIDATES else "full"),
                                      "single:%s" % ("sorted" if a["sorted"] else "unsorted")]
    offsets_form = step["call"] == "run_batch_offsets_ptr"
    plan = g.plan_top_k_batch(a["total"] if offsets_form else a["count"], a["num_segments"] if offsets_form else a["num_partitions"], a["k"],
                              a["key_type"], offsets_form, a["sorted"], bool(a["outputs"][0] or a["outputs"][1]), a["loop_min"])
    kb = np.dtype(a["key_type"]).itemsize
    out = []
    if plan["path"] == BINNED:
        out += ["binned:" + c for c in ("wave", "block", "long") if d.get(c)]
    elif plan["path"]:
        out.append("equal:" + ("", "wave", "block", "long", "loop")[plan["path"]])
    if plan["path"] and a["sorted"] and (a["outputs"][0] or a["outputs"][1]):
        out.append("rows:%s" % ("one_sort_per_row" if g.plan_batch(a["k"], kb, True)[0] == 3 else "batched_sort"))
    return out


def required_top_k():
    return ["single:candidates", "single:full", "single:sorted", "single:unsorted", "binned:wave", "binned:block", "binned:long", "equal:wave",
            "equal:block", "equal:long", "equal:loop", "rows:batched_sort", "rows:one_sort_per_row"]


# ---------------------------------------------------------------------------------------------------------------- the table of units

TABLE = {
    "RadixSort": (gen_radix_sort, exp_radix_sort, diag_radix_sort, classes_radix_sort, required_radix_sort),
    "BlellochScan": (gen_scan, exp_scan, diag_scan, classes_scan, required_scan),
    "Reduce": (gen_reduce, exp_reduce, diag_reduce, classes_reduce, required_reduce),
    "KeyRuns": (gen_key_runs, exp_key_runs, lambda step: {}, classes_key_runs, required_key_runs),
    "Select": (gen_select, exp_select, lambda step: {}, classes_select, required_select),
    "SortedSearch": (gen_sorted_search, exp_sorted_search, diag_sorted_search, classes_sorted_search, required_sorted_search),
    "Merge": (gen_merge, exp_merge, diag_merge, classes_merge, required_merge),
    "SetOps": (gen_set_ops, exp_set_ops, diag_set_ops, classes_set_ops, required_set_ops),
    "Histogram": (gen_histogram, exp_histogram, diag_histogram, classes_histogram, required_histogram),
    "Expand": (gen_expand, exp_expand, diag_expand, classes_expand, required_expand),
    "Gather": (gen_gather, exp_gather, diag_gather, classes_gather, required_gather),
    "TopK": (gen_top_k, exp_top_k, diag_top_k, classes_top_k, required_top_k),
}


def sequence(unit, seed, steps=STEPS):
    """The fully drawn steps of one sequence on the objects of `unit`."""
    rng = np.random.default_rng([seed, UNITS.index(unit)])
    return TABLE[unit][0](G(), rng, unit, seed, steps)


def expected(step):
    """{array name: contents after the call} for every array of the step that the call may write; numpy only."""
    return TABLE[step["unit"]][1](step)


def expected_diag(step):
    """What the object must report about the call (last(), read_last(), read_batch()), from the host-only plan functions."""
    return TABLE[step["unit"]][2](step)


def classes(step):
    """The classes and paths of the unit that the step reaches, by the plan functions."""
    return TABLE[step["unit"]][3](step)


def required_classes(unit):
    return TABLE[unit][4]()


# ---------------------------------------------------------------------------------------------------------------- the device side


def make_object(g, step):
    """The long-lived object a step runs on, by its name in the step."""
    kind = step["obj"].split(":")
    if kind[0] == "sort":
        return g.RadixSort()
    if kind[0] == "reduce":
        return g.Reduce(int(kind[1]), int(kind[2]))
    if kind[0] == "scan":
        return g.BlellochScan(int(kind[1]))
    if kind[0] == "runs":
        return {"runs": g.KeyRuns(), "reduce": g.Reduce(g.DataType_Uint, g.ReduceOperator_Sum), "scan": g.BlellochScan(g.DataType_Uint)}
    return {"select": g.Select, "search": g.SortedSearch, "merge": g.Merge, "set_ops": g.SetOps, "histogram": g.Histogram, "expand": g.Expand,
            "gather": g.Gather, "top_k": g.TopK}[kind[0]]()


def prepare_objects(g, steps, objects):
    """One prepare per object and shape for the maximum over the sequence; returns a function that reads what must not move after."""
    unit = steps[0]["unit"]
    for s in steps:
        objects.setdefault(s["obj"], make_object(g, s))
    most = lambda key: max([s["args"].get(key, 0) for s in steps] + [0])  # noqa: E731
    size = max(s["size"] for s in steps) + 8
    if unit == "RadixSort":
        sorter = objects["sort"]
        for kb in (4, 8):
            for with_vals in (True, False):
                sorter.prepare_batch(size, max(most("num_segments"), most("num_partitions"), 1), kb, with_vals)
                sorter.prepare_internal_buffers(size, kb, with_vals)
        return sorter.scratch_size
    if unit in ("BlellochScan", "Reduce"):
        for s in steps:
            rows = s["size"] * 4 // elem_bytes(s["args"]["data_type"]) + 8
            objects[s["obj"]].prepare_batch(rows, max(s["args"].get("num_segments", 0), s["args"].get("num_partitions", 0), 1))
            if s["call"] == "run_ptr":
                objects[s["obj"]].prepare(s["args"]["count"], s["args"]["num_partitions"])
    elif unit == "KeyRuns":
        for bits in (32, 64):
            objects["runs"]["runs"].prepare(size, bits)
        objects["runs"]["reduce"].prepare_batch(size, most("max_runs"))
        objects["runs"]["scan"].prepare_batch(size, most("max_runs"))
    elif unit == "Select":
        for st in STENCILS:
            objects["select"].prepare(size, st)
    elif unit == "SortedSearch":
        for s in steps:
            objects["search"].set_option("TOP_ENTRIES", s["args"]["top_entries"])
            objects["search"].prepare(s["args"]["hay_count"], s["args"]["key_type"])
    elif unit in ("Merge", "SetOps"):
        for kt in KEY_TYPES:
            objects[steps[0]["obj"]].prepare(size, kt)
    elif unit == "Histogram":
        objects["histogram"].prepare(size, 8192)
    elif unit == "Expand":
        objects["expand"].prepare(size, most("num_segments"))
    elif unit == "TopK":
        for kt in KEY_TYPES:
            objects["top_k"].prepare(size, most("k"), kt)
            objects["top_k"].prepare_batch(size, max(most("num_segments"), most("num_partitions"), 1), most("k"), kt)
    return None


def invoke(g, obj, step, ptr, stream):
    """The one library call of a step (KeyRuns by key: the two calls the binding composes), on `stream`."""
    a, call, unit = step["args"], step["call"], step["unit"]
    if unit == "RadixSort":
        if call == "sort_batch_offsets_ptr":
            obj.sort_batch_offsets_ptr(ptr("keys"), ptr("vals"), a["total"], ptr("offsets"), a["num_segments"], a["key_type"], stream)
        elif call == "sort_batch_ptr":
            obj.sort_batch_ptr(ptr("keys"), ptr("vals"), a["count"], a["num_partitions"], a["key_type"], stream)
        elif call == "sort_typed_ptr":
            obj.sort_typed_ptr(ptr("keys"), ptr("vals"), a["count"], a["key_type"], stream)
        elif call == "sort_keys_ptr":
            obj.sort_keys_ptr(ptr("keys"), a["count"], 0, stream, np.dtype(a["key_type"]).itemsize)
        else:
            obj.sort_bit_range_ptr(ptr("keys"), ptr("vals"), a["count"], a["begin_bit"], a["end_bit"], stream, np.dtype(a["key_type"]).itemsize)
    elif unit == "Reduce":
        if call == "run_batch_offsets_ptr":
            obj.run_batch_offsets_ptr(ptr("data"), ptr("out"), a["total"], ptr("offsets"), a["num_segments"], stream)
        else:
            obj.run_batch_ptr(ptr("data"), ptr("out"), a["count"], a["num_partitions"], stream)
    elif unit == "BlellochScan":
        if call == "run_batch_offsets_ptr":
            obj.run_batch_offsets_ptr(ptr("data"), a["total"], ptr("offsets"), a["num_segments"], stream)
        else:
            obj.run_ptr(ptr("data"), a["count"], a["num_partitions"], stream)
    elif unit == "KeyRuns":
        common = dict(unique_keys_ptr=ptr("unique_keys"), key_bits=a["key_bits"], begin_bit=a["begin_bit"], end_bit=a["end_bit"], stream=stream)
        if call == "run_ptr":
            obj["runs"].run_ptr(ptr("keys"), a["count"], ptr("offsets"), a["max_runs"], ptr("num_runs"), **common)
        elif call == "reduce_by_key":
            obj["reduce"].run_by_key_ptr(obj["runs"], ptr("keys"), ptr("values"), ptr("out"), a["count"], ptr("offsets"), a["max_runs"],
                                         ptr("num_runs"), **common)
        else:
            obj["scan"].run_by_key_ptr(obj["runs"], ptr("keys"), ptr("values"), a["count"], ptr("offsets"), a["max_runs"], ptr("num_runs"),
                                       **common)
    elif unit == "Select":
        obj.run_ptr(ptr("stencil"), a["count"], a["max_out"], ptr("num_selected"), ptr("out_indices"), ptr("items"), ptr("out_items"),
                    a["item_bytes"] or 4, a["stencil_type"], a["op"], a["threshold"], stream)
    elif unit == "SortedSearch":
        if call == "index_ptr":
            obj.index_ptr(ptr("hay"), a["hay_count"], a["key_type"], stream)
        else:
            obj.run_ptr(ptr("hay"), a["hay_count"], ptr("needles"), a["needle_count"], ptr("out_lower"), ptr("out_upper"), a["key_type"],
                        a["reuse_index"], stream)
    elif unit == "Merge":
        obj.run_ptr(ptr("a_keys"), ptr("a_vals"), a["a_count"], ptr("b_keys"), ptr("b_vals"), a["b_count"], ptr("out_keys"), ptr("out_vals"),
                    a["key_type"], stream)
    elif unit == "SetOps":
        obj.run_ptr(a["op"], ptr("a_keys"), ptr("a_vals"), a["a_count"], ptr("b_keys"), ptr("b_vals"), a["b_count"], ptr("out_keys"),
                    ptr("out_vals"), a["max_out"], ptr("num_out"), a["key_type"], stream)
    elif unit == "Histogram":
        if call == "run_even_ptr":
            obj.run_even_ptr(ptr("samples"), a["count"], a["lo"], a["hi"], a["bins"], ptr("counts"), a["key_type"], a["accumulate"], stream)
        else:
            obj.run_edges_ptr(ptr("samples"), a["count"], ptr("edges"), a["bins"], ptr("counts"), a["key_type"], a["accumulate"], stream)
    elif unit == "Expand":
        obj.run_ptr(ptr("offsets"), a["num_segments"], a["total"], ptr("out_segments"), ptr("out_ranks"), ptr("items"), ptr("out_items"),
                    a["item_bytes"], stream)
    elif unit == "Gather":
        ib = a["item_bytes"]
        if call == "run_ptr":
            obj.run_ptr(ptr("items"), a["item_count"], ib, ptr("indices"), a["count"], ptr("out"), stream)
        elif call == "scatter_ptr":
            obj.scatter_ptr(ptr("items"), ib, ptr("indices"), a["count"], ptr("out"), a["out_count"], stream)
        elif call == "run_batch_ptr":
            obj.run_batch_ptr(ptr("items"), ib, a["count"], a["num_partitions"], ptr("indices"), a["k"], ptr("out"), stream)
        else:
            obj.run_batch_offsets_ptr(ptr("items"), ib, a["total"], ptr("offsets"), a["num_segments"], ptr("indices"), a["k"], ptr("out"), stream)
    elif unit == "TopK":
        outs = dict(out_keys_ptr=ptr("out_keys"), out_indices_ptr=ptr("out_indices"), out_kth_ptr=ptr("out_kth"), key_type=a["key_type"],
                    largest=a["largest"], sorted=a["sorted"], stream=stream)
        if call == "run_ptr":
            obj.run_ptr(ptr("keys"), a["count"], a["k"], **outs)
        elif call == "run_batch_ptr":
            obj.run_batch_ptr(ptr("keys"), a["count"], a["num_partitions"], a["k"], **outs)
        else:
            obj.run_batch_offsets_ptr(ptr("keys"), a["total"], ptr("offsets"), a["num_segments"], a["k"], **outs)
    else:
        raise ValueError(unit)


def read_diag(obj, step):
    """The object's own account of its last call, in the shape of expected_diag."""
    unit, call = step["unit"], step["call"]
    if unit == "RadixSort":
        return obj.read_batch() if call.startswith("sort_batch") else {}
    if unit == "Reduce" or (unit == "BlellochScan" and call == "run_batch_offsets_ptr"):
        return obj.read_batch()
    if unit in ("SortedSearch", "Merge", "SetOps", "Histogram", "Expand", "Gather"):
        return {"last": obj.last()}
    if unit == "TopK":
        return obj.read_last() if call == "run_ptr" else obj.read_batch()
    return {}


def run_sequence(g, steps, prepared, stream=None, on_result=None):
    """Runs the steps in order on one set of objects and one stream; raises Mismatch (or GluError) at the first step that differs.
    Returns the images of every step (for a comparison between two runs)."""
    import torch

    stream = stream or torch.cuda.current_stream()
    objects, kept, all_images = {}, {}, []
    fixed = prepare_objects(g, steps, objects) if prepared else None
    before = fixed() if fixed else None
    with torch.cuda.stream(stream):
        for step in steps:
            if step["obj"] not in objects:
                objects[step["obj"]] = make_object(g, step)
            obj = objects[step["obj"]]
            for _, name, value in step["options"]:
                obj.set_option(name, value)
            buffers = {}
            for name, a in step["arrays"].items():
                if a.get("carry") and name in kept:
                    buffers[name] = kept[name]
                else:
                    buffers[name] = torch.from_numpy(image(a)).cuda()
                    assert buffers[name].data_ptr() % 16 == 0
            kept = buffers

            def ptr(name):
                return buffers[name].data_ptr() + GUARD + step["arrays"][name]["shift"] if name in buffers else None

            invoke(g, obj, step, ptr, stream.cuda_stream)
            if stream.cuda_stream:
                stream.synchronize()
            else:  # (the default stream's handle is NULL, which the library reads as its own queue: wait for the device)
                torch.cuda.synchronize()
            images = {name: t.cpu().numpy() for name, t in buffers.items()}
            check(step, images, read_diag(obj, step))
            if fixed and fixed() != before:
                raise Mismatch("%r: a prepared object's scratch moved from %d to %d bytes" % (scalars(step), before, fixed()))
            all_images.append(images)
    return all_images


def threads_child():
    """Four host threads, each with its own objects of one unit and its own stream, the first twelve steps of that unit's sequence
    each; the first library call of the process happens behind the barrier, in all four at once.  Exit status 0: all agree."""
    import threading

    import torch

    units = ("RadixSort", "TopK", "Merge", "Reduce")
    work = {u: sequence(u, SEEDS[u][0])[:12] for u in units}  # (plan functions only: no device, no one-time setup of a kernel)
    g = G()
    barrier = threading.Barrier(len(units))
    failures = []

    def body(unit):
        try:
            barrier.wait(timeout=60)
            torch.cuda.set_device(0)
            run_sequence(g, work[unit], False, torch.cuda.Stream())
            print("thread %s: 12 steps agree" % unit, flush=True)
        except BaseException as e:  # noqa: B902
            failures.append((unit, repr(e)))

    threads = [threading.Thread(target=body, args=(u,), name=u) for u in units]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
        if t.is_alive():
            failures.append((t.name, "did not join"))
    for f in failures:
        print("FAILED", f, flush=True)
    os._exit(1 if failures else 0)  # (a thread that did not join must not keep the process)


if __name__ == "__main__":
    if sys.argv[1:] == ["threads"]:
        threads_child()
