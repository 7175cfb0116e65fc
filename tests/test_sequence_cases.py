"""CPU tests of the generator of call sequences (sequence_cases.py) and of its checker: the committed seeds give the same steps every
time, every step satisfies the preconditions of its call, the order conditions that make a sequence worth running hold, the two
sequences of a unit reach every class and path the plan functions know at these sizes, and the checker rejects doctored results.  No
device: the plan functions of the library are host code."""
import collections

import numpy as np
import pytest

import sequence_cases as sc
from test_top_k_pick import key_code


@pytest.fixture(scope="module")
def sequences(built):
    return {(unit, seed): sc.sequence(unit, seed) for unit in sc.UNITS for seed in sc.SEEDS[unit]}


@pytest.mark.parametrize("unit", sc.UNITS)
def test_the_committed_seeds_give_the_same_steps_again(sequences, unit):
    for seed in sc.SEEDS[unit]:
        steps = sequences[unit, seed]
        assert len(steps) == sc.STEPS
        assert sc.step_hash(sc.sequence(unit, seed)) == sc.step_hash(steps)
    assert sc.step_hash(sequences[unit, sc.SEEDS[unit][0]]) != sc.step_hash(sequences[unit, sc.SEEDS[unit][1]])


def is_sorted(keys):
    code = key_code(keys, False)
    return bool((code[1:] >= code[:-1]).all())


def monotone_within(offsets, total):
    o = offsets.astype(np.int64)
    return bool((np.diff(o) >= 0).all() and o[-1] <= total)


@pytest.mark.parametrize("unit", sc.UNITS)
def test_every_step_satisfies_the_preconditions_of_its_call(sequences, unit):
    for seed in sc.SEEDS[unit]:
        last_index = None
        for step in sequences[unit, seed]:
            a, arrays, what = step["args"], step["arrays"], sc.scalars(step)
            for name, arr in arrays.items():  # shifts: multiples of the alignment the header asks for, inside one 16-byte pack
                assert 0 <= arr["shift"] < 16, (what, name)
            if "offsets" in arrays and unit != "KeyRuns":
                total = a["total"] if unit != "Expand" else 2 ** 32
                assert monotone_within(arrays["offsets"]["data"], total), what
                assert arrays["offsets"]["data"].size == a["num_segments"] + 1 <= (1 << 24) + 1, what
            for name in ("keys", "data", "stencil", "hay", "needles", "a_keys", "b_keys", "samples", "edges"):
                if name in arrays:
                    assert arrays[name]["shift"] % arrays[name]["data"].dtype.itemsize == 0, (what, name)
            if unit in ("Merge", "SetOps"):
                assert is_sorted(arrays["a_keys"]["data"]) and is_sorted(arrays["b_keys"]["data"]), what
                assert ("a_vals" in arrays) == ("out_vals" in arrays), what
                if unit == "SetOps":
                    assert a["max_out"] > 0 or "out_keys" not in arrays, what
            if unit == "SortedSearch":
                assert is_sorted(arrays["hay"]["data"]), what
                F = sc.fanout(a["key_type"])
                assert F <= a["top_entries"] <= (8192 if F == 32 else 4096), what
                if a["reuse_index"]:  # the haystack, its count, its type and TOP_ENTRIES are those of the index built last
                    assert last_index is not None and last_index[1:] == (a["key_type"], a["hay_count"], a["top_entries"]), what
                    assert arrays["hay"].get("carry") and arrays["hay"]["data"] is last_index[0], what
                else:
                    built = sc.expected_diag(step).get("last", (0, 0, 0))
                    builds = built[0] == sc.INDEXED and built[2] == (1 if step["call"] == "index_ptr" else 2)
                    last_index = (arrays["hay"]["data"], a["key_type"], a["hay_count"], a["top_entries"]) if builds else None
                if step["call"] == "run_ptr":
                    assert "out_lower" in arrays or "out_upper" in arrays, what
            if unit == "TopK":
                if step["call"] != "run_batch_offsets_ptr":
                    assert a["k"] <= a["count"], what
                assert any(a["outputs"]) and (a["k"] > 0 or step["call"] == "run_ptr"), what
                rows = a.get("num_segments", a.get("num_partitions", 1))
                assert rows * a["k"] < 2 ** 32 and rows <= 1 << 24, what
            if unit == "Histogram":
                assert 1 <= a["bins"] <= (8192 if a["mode"] == "edges" else 1 << 24), what
                if a["mode"] == "edges":
                    e = arrays["edges"]["data"]
                    assert e.size == a["bins"] + 1 and not (e.dtype.kind == "f" and np.isnan(e).any()) and (e[1:] >= e[:-1]).all(), what
                elif arrays["samples"]["data"].dtype.kind == "f":
                    assert np.isfinite([a["lo"], a["hi"]]).all() and a["lo"] < a["hi"], what
                else:
                    assert a["key_type"] in ("uint32", "int32") and (a["hi"] - a["lo"]) % a["bins"] == 0 and a["hi"] > a["lo"], what
                    info = np.iinfo(a["key_type"])
                    assert info.min <= a["lo"] and a["hi"] <= info.max, what
            if unit == "Select":
                assert a["item_bytes"] in (0, 4, 8, 16, 32) and 0 <= a["op"] < 6, what
            if unit == "KeyRuns":
                assert 0 <= a["begin_bit"] <= a["end_bit"] <= a["key_bits"] and 1 <= a["max_runs"] <= 1 << 24, what
            if unit == "Gather" and step["call"] == "scatter_ptr":
                idx = arrays["indices"]["data"]
                valid = idx[idx < a["out_count"]]
                assert np.unique(valid).size == valid.size, what  # distinct where they are in range: the result is determined
            if unit == "BlellochScan" and step["call"] == "run_ptr":
                assert a["count"] > 0 and a["num_partitions"] >= 1 and a["count"] * a["num_partitions"] < 1 << 23, what
            if unit == "RadixSort" and not step["call"].startswith("sort_batch"):
                assert a["count"] > 0, what
                if step["call"] == "sort_bit_range_ptr":
                    assert 0 <= a["begin_bit"] < a["end_bit"] <= 8 * np.dtype(a["key_type"]).itemsize, what
            for name, want in sc.expected(step).items():  # the answer has the shape of the array it describes
                assert want.nbytes == arrays[name]["data"].nbytes and arrays[name]["role"] != "in", (what, name)


@pytest.mark.parametrize("unit", sc.UNITS)
def test_the_order_of_the_steps_is_what_the_sequences_are_for(sequences, unit):
    """At least 8 steps at most a quarter of the largest before them, at least 8 changes of the key or data type (the width among
    them), at least 6 changes of an option or of the set of optional outputs."""
    for seed in sc.SEEDS[unit]:
        steps = sequences[unit, seed]
        largest, small = 0, 0
        for s in steps:
            small += largest > 0 and 4 * s["size"] <= largest
            largest = max(largest, s["size"])
        types = sum(a["type"] != b["type"] for a, b in zip(steps, steps[1:]))
        variants = sum(a["variant"] != b["variant"] for a, b in zip(steps, steps[1:]))
        assert small >= 8 and types >= 8 and variants >= 6, (unit, seed, small, types, variants)
        widths = {np.asarray(a["data"]).dtype.itemsize for s in steps for n, a in s["arrays"].items() if n in ("keys", "hay", "a_keys", "samples")}
        if unit in ("RadixSort", "SortedSearch", "Merge", "SetOps", "TopK", "Histogram", "KeyRuns"):
            assert widths == {4, 8}, (unit, seed, widths)


def test_float_sums_and_products_are_exact_in_any_order(sequences):
    """Reduce: the reference folded forwards, backwards and as a balanced tree gives the same bits for every segment; BlellochScan:
    prefixes added up from the front equal the total less the suffix added up from the back."""
    floats = 0
    for unit in ("Reduce", "BlellochScan"):
        for seed in sc.SEEDS[unit]:
            for step in sequences[unit, seed]:
                name, comps = sc.DATA_TYPES[step["args"]["data_type"]]
                fn = sc.exp_reduce if unit == "Reduce" else sc.exp_scan
                forward = fn(step)
                for order in ("backward", "pairwise") if unit == "Reduce" else ("backward",):
                    other = fn(step, order)
                    for key in forward:
                        assert forward[key].tobytes() == other[key].tobytes(), (sc.scalars(step), order)
                if np.dtype(name).kind == "f":
                    floats += 1
                    data = step["arrays"]["data"]["data"]
                    assert not np.isnan(data).any() and not (np.signbit(data) & (data == 0)).any(), sc.scalars(step)
    assert floats >= 20


def test_every_class_and_path_is_reached_at_least_twice(sequences):
    table = {}
    for unit in sc.UNITS:
        reached = collections.Counter()
        for seed in sc.SEEDS[unit]:
            for step in sequences[unit, seed]:
                reached.update(set(sc.classes(step)))
        table[unit] = reached
    print()
    print("%-14s %-28s %s" % ("unit", "class or path", "steps that reach it"))
    for unit in sc.UNITS:
        for name in sorted(set(table[unit]) | set(sc.required_classes(unit))):
            print("%-14s %-28s %d" % (unit, name, table[unit][name]))
    missing = [(unit, name, table[unit][name]) for unit in sc.UNITS for name in sc.required_classes(unit) if table[unit][name] < 2]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------- the checker


def faithful(step):
    return {name: img.copy() for name, img in sc.expected_images(step).items()}


def find_step(sequences, unit, pred):
    for seed in sc.SEEDS[unit]:
        for step in sequences[unit, seed]:
            if pred(step):
                return step
    raise AssertionError("no step of %s to doctor" % unit)


def inside(step, name, element, dtype):
    """A view of the bytes of element `element` of array `name` inside its image."""
    a = step["arrays"][name]
    lo = sc.GUARD + a["shift"] + element * np.dtype(dtype).itemsize
    return slice(lo, lo + np.dtype(dtype).itemsize)


@pytest.mark.parametrize("unit", sc.UNITS)
def test_the_checker_accepts_the_answer_itself_and_rejects_a_flipped_guard_and_a_changed_input(sequences, unit):
    for seed in sc.SEEDS[unit]:
        for step in sequences[unit, seed]:
            sc.check(step, faithful(step))
            for name, a in step["arrays"].items():
                for at in (0, sc.GUARD + a["shift"] - 1, sc.GUARD + a["shift"] + a["data"].nbytes, -1):  # both guards, both ends of each
                    doctored = faithful(step)
                    doctored[name][at] ^= 1
                    with pytest.raises(sc.Mismatch, match="guard"):
                        sc.check(step, doctored)
                if a["role"] == "in" and a["data"].nbytes:
                    doctored = faithful(step)
                    doctored[name][sc.GUARD + a["shift"] + a["data"].nbytes // 2] ^= 0x10
                    with pytest.raises(sc.Mismatch, match="input"):
                        sc.check(step, doctored)


def test_the_checker_rejects_two_values_swapped_among_equal_keys(sequences):
    def has_tie(step):
        if not step["args"]["with_vals"]:
            return False
        k, v = sc.expected(step)["out_keys"], sc.expected(step)["out_vals"]
        return k.size > 1 and bool(((k.view(sc.uint_of(k.dtype))[1:] == k.view(sc.uint_of(k.dtype))[:-1]) & (v[1:] != v[:-1])).any())

    step = find_step(sequences, "Merge", has_tie)
    k, v = sc.expected(step)["out_keys"], sc.expected(step)["out_vals"]
    u = k.view(sc.uint_of(k.dtype))
    at = int(np.flatnonzero((u[1:] == u[:-1]) & (v[1:] != v[:-1]))[0])
    doctored = faithful(step)
    first, second = inside(step, "out_vals", at, np.uint32), inside(step, "out_vals", at + 1, np.uint32)
    doctored["out_vals"][first], doctored["out_vals"][second] = doctored["out_vals"][second].copy(), doctored["out_vals"][first].copy()
    with pytest.raises(sc.Mismatch, match="out_vals differs in its contents"):
        sc.check(step, doctored)


@pytest.mark.parametrize("unit, name", [("SetOps", "num_out"), ("Select", "num_selected"), ("KeyRuns", "num_runs")])
def test_the_checker_rejects_a_count_off_by_one(sequences, unit, name):
    step = find_step(sequences, unit, lambda s: True)
    for delta in (1, -1):
        doctored = faithful(step)
        word = doctored[name][inside(step, name, 0, np.uint32)].view(np.uint32)
        word += np.uint32(delta & 0xFFFFFFFF)
        with pytest.raises(sc.Mismatch, match=name):
            sc.check(step, doctored)


@pytest.mark.parametrize("unit, name, length", [("SetOps", "out_keys", lambda s: min(s["args"]["kept"], s["args"]["max_out"])),
                                                ("Select", "out_indices", lambda s: min(s["args"]["selected"], s["args"]["max_out"])),
                                                ("TopK", "out_keys", lambda s: s["args"]["k"])])
def test_the_checker_rejects_a_stale_element_behind_the_written_length(sequences, unit, name, length):
    """What an earlier, longer call left in a scratch array and a kernel then copied out: one plausible element just behind the end."""
    step = find_step(sequences, unit, lambda s: name in s["arrays"] and s["call"] == "run_ptr" and 0 < length(s)
                     and s["arrays"][name]["data"].size > length(s))
    dtype = step["arrays"][name]["data"].dtype
    doctored = faithful(step)
    doctored[name][inside(step, name, length(step), dtype)] = doctored[name][inside(step, name, length(step) - 1, dtype)]
    with pytest.raises(sc.Mismatch, match=name + " differs in its contents"):
        sc.check(step, doctored)


def test_the_checker_rejects_an_account_that_is_not_the_plans(sequences):
    step = find_step(sequences, "Merge", lambda s: s["size"] > 0)
    tiles, kernels = sc.expected_diag(step)["last"]
    sc.check(step, faithful(step), {"last": (tiles, kernels)})
    with pytest.raises(sc.Mismatch, match="the plan says"):
        sc.check(step, faithful(step), {"last": (tiles + 1, kernels)})
