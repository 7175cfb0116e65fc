"""CPU test of what a sort call decides on the host before it enqueues anything (csrc/sort_call_plan.hpp): the list of its passes --
digit positions, key transforms, which passes share a count kernel, the two top-bit passes of an attempt to end in LDS in front -- and
whether the call attempts, given the object's memory of its earlier attempts and the five hint words the device wrote.  The header is
plain C++: a host program runs the two functions on cases from a file, an attempt's feedback as a sequence of calls with scripted hint
words, and writes what they returned and every state field.  The expected values are written out here from the rules.  The same
program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SIGNED, FLOAT = 1, 2  # (radix_sort_kernels.hpp: KEY_XF_SIGNED, KEY_XF_FLOAT; the decode bits are these << 2)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sort_call_plan.hpp"
using namespace glu_hip;

static FILE* in;
static FILE* out;
static unsigned get()
{
    unsigned v = 0;
    if (fscanf(in, "%u", &v) != 1) exit(3);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "r");
    out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    const unsigned cases = get();
    for (unsigned c = 0; c < cases; c++)
    {
        const unsigned kind = get();
        if (kind == 0) // a pass list
        {
            unsigned a[10];
            for (unsigned& x : a) x = get();
            // (on the heap, exactly as long as the list: the sanitizers see a write past its end)
            std::vector<SortPassList> list(1);
            const bool ok = sort_call_passes(list[0], a[0], a[1], a[2], a[3], a[4], a[5] != 0, a[6], a[7] != 0, a[8] != 0, a[9] != 0);
            fprintf(out, "%d %u", ok ? 1 : 0, list[0].num);
            for (unsigned p = 0; ok && p < list[0].num; p++)
                fprintf(out, " %u %u %u %d", list[0].passes[p].shift, list[0].passes[p].bits, list[0].passes[p].xform, list[0].passes[p].pair_role);
            fprintf(out, "\n");
        }
        else // the feedback of an attempt: a state, then calls
        {
            const unsigned device_top = get(), key_bytes = get(), end_bit = get();
            FinishFeedback f;
            f.finish_seq = get(), f.finish_seq_acted_on = get(), f.finish_wait = get(), f.finish_last_geo = get();
            f.finish_last_refused = get() != 0;
            f.top_floor = get(), f.finish_top = get(), f.finish_backoff = get();
            const unsigned calls = get();
            for (unsigned i = 0; i < calls; i++)
            {
                const bool have = get() != 0;
                std::vector<uint32_t> hint(5); // (on the heap: see above)
                for (uint32_t& w : hint) w = get();
                const bool attempts = finish_attempts(f, have ? hint.data() : nullptr, device_top != 0, key_bytes, end_bit);
                fprintf(out, "%d %u %u %u %u %d %u %u %u\n", attempts ? 1 : 0, f.finish_seq, f.finish_seq_acted_on, f.finish_wait, f.finish_last_geo,
                        f.finish_last_refused ? 1 : 0, f.top_floor, f.finish_top, f.finish_backoff);
            }
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}
"""

# ---- the cases -------------------------------------------------------------------------------------------------------------------


def passes(key_bytes, first_bit, end_bit, digit_bits, key_xf=0, attempt=False, top=0, pairs_ok=False, lines8=True, lines4=True):
    return (0, key_bytes, first_bit, end_bit, digit_bits, key_xf, int(attempt), top, int(pairs_ok), int(lines8), int(lines4))


def P(shift, bits, xform=0, role=0):
    return (shift, bits, xform, role)


PASS_CASES = {
    "whole 32-bit key, 8-bit digits": (passes(4, 0, 32, 8), [P(0, 8), P(8, 8), P(16, 8), P(24, 8)]),
    "whole 32-bit key, 4-bit digits": (passes(4, 0, 32, 4), [P(s, 4) for s in (0, 4, 8, 12, 16, 20, 24, 28)]),
    "64-bit key, bits [28, 36): no digit straddles bit 32": (passes(8, 28, 36, 8), [P(28, 4), P(32, 4)]),
    "64-bit key, bits [30, 48), 4-bit digits: the word's last digit is cut": (passes(8, 30, 48, 4), [P(30, 2), P(32, 4), P(36, 4), P(40, 4), P(44, 4)]),
    "32-bit key: nothing is cut at bit 32 of a key that ends there": (passes(4, 28, 32, 8), [P(28, 4)]),
    "odd remainder": (passes(4, 0, 20, 8), [P(0, 8), P(8, 8), P(16, 4)]),
    "signed keys: encode on the first pass, decode on the last": (passes(4, 0, 32, 8, SIGNED),
                                                                  [P(0, 8, SIGNED), P(8, 8), P(16, 8), P(24, 8, SIGNED << 2)]),
    "float keys, 64 bits": (passes(8, 0, 64, 8, FLOAT), [P(0, 8, FLOAT)] + [P(s, 8) for s in range(8, 56, 8)] + [P(56, 8, FLOAT << 2)]),
    "typed keys, one pass: both": (passes(4, 0, 8, 8, FLOAT), [P(0, 8, FLOAT | FLOAT << 2)]),
    "typed keys, one pass of a bit range": (passes(4, 5, 9, 8, SIGNED), [P(5, 4, SIGNED | SIGNED << 2)]),
    "ordinary passes pair from pairs_ok": (passes(4, 0, 32, 8, pairs_ok=True), [P(0, 8, 0, 1), P(8, 8, 0, 2), P(16, 8, 0, 1), P(24, 8, 0, 2)]),
    "typed keys: the first pass encodes and is no leader": (passes(4, 0, 32, 8, SIGNED, pairs_ok=True),
                                                            [P(0, 8, SIGNED), P(8, 8, 0, 1), P(16, 8, 0, 2), P(24, 8, SIGNED << 2)]),
    "an attempt, untyped, pairs_ok": (passes(4, 0, 32, 8, attempt=True, top=32, pairs_ok=True),
                                      [P(16, 8, 0, 1), P(24, 8, 0, 2), P(0, 8, 0, 1), P(8, 8, 0, 2), P(16, 8, 0, 1), P(24, 8, 0, 2)]),
    "an attempt below a guessed top bit": (passes(4, 0, 32, 8, attempt=True, top=28, pairs_ok=True),
                                           [P(12, 8, 0, 1), P(20, 8, 0, 2), P(0, 8, 0, 1), P(8, 8, 0, 2), P(16, 8, 0, 1), P(24, 8, 0, 2)]),
    "an attempt without pairs_ok: only its two passes pair": (passes(4, 0, 32, 8, attempt=True, top=32),
                                                              [P(16, 8, 0, 1), P(24, 8, 0, 2), P(0, 8), P(8, 8), P(16, 8), P(24, 8)]),
    "an attempt on 64-bit keys": (passes(8, 0, 64, 8, attempt=True, top=48),
                                  [P(32, 8, 0, 1), P(40, 8, 0, 2)] + [P(s, 8) for s in range(0, 64, 8)]),
    # pass 0 encodes and leads all the same; pass 2, the ordinary first pass, encodes and does not; 3 and 4 pair; 5 has no partner
    "an attempt on typed keys": (passes(4, 0, 32, 8, SIGNED, attempt=True, top=32, pairs_ok=True),
                                 [P(16, 8, SIGNED, 1), P(24, 8, 0, 2), P(0, 8, SIGNED), P(8, 8, 0, 1), P(16, 8, 0, 2), P(24, 8, SIGNED << 2)]),
    "a mixed tail: the last pass has no partner of its width": (passes(4, 0, 20, 8, pairs_ok=True), [P(0, 8, 0, 1), P(8, 8, 0, 2), P(16, 4)]),
    "two passes of different widths do not pair": (passes(4, 0, 12, 8, pairs_ok=True), [P(0, 8), P(8, 4)]),
    "4-bit digits pair by the 4-bit line kernel": (passes(4, 0, 16, 4, pairs_ok=True, lines8=False),
                                                   [P(0, 4, 0, 1), P(4, 4, 0, 2), P(8, 4, 0, 1), P(12, 4, 0, 2)]),
    "lines4 false with 4-bit digits: no pairs": (passes(4, 0, 32, 4, pairs_ok=True, lines4=False), [P(s, 4) for s in range(0, 32, 4)]),
    "lines8 false with 8-bit digits: no pairs": (passes(4, 0, 32, 8, pairs_ok=True, lines8=False), [P(s, 8) for s in range(0, 32, 8)]),
    "first_bit == end_bit: no passes": (passes(4, 8, 8, 8, pairs_ok=True), []),
    "first_bit > end_bit: no passes": (passes(8, 40, 8, 8, SIGNED), []),
    # 64-bit keys in 4-bit digits: 16 passes, as many as any call asks for (a plan holds 32); from bit 1, one digit is cut at bit 32
    "the longest list": (passes(8, 1, 64, 4), [P(s, 4) for s in range(1, 29, 4)] + [P(29, 3)] + [P(s, 4) for s in range(32, 64, 4)]),
}

ZERO = dict(seq=0, acted=0, wait=0, geo=0, refused=0, floor=0, top=0, backoff=0)
FIELDS = ("seq", "acted", "wait", "geo", "refused", "floor", "top", "backoff")


def state(**kw):
    s = dict(ZERO)
    s.update(kw)
    return s


def word0(seq, geo):
    return seq << 3 | geo


def bits(n):
    """(word 1, word 2): the low n key bits vary."""
    v = (1 << n) - 1
    return v & 0xFFFFFFFF, v >> 32


def hint(w0=0, varying=(0, 0), valid_for=0, used=0):
    return (w0, varying[0], varying[1], valid_for, used)


def feedback(device_top, key_bytes, end_bit, start, calls):
    """calls: [(hint words or None, attempts, the fields that differ from the state before the call)]"""
    return (device_top, key_bytes, end_bit, start, calls)


def backoff_calls(seq, backoff, first_hint, first_changes):
    """A refusal that is acted on with back-off N: that call and the N - 1 behind it do not attempt while finish_wait counts down to
    0; the call after them sees the same outcome, does not act on it again, and attempts."""
    calls = [(first_hint, 0, dict(first_changes, wait=backoff - 1))]
    calls += [(first_hint, 0, dict(wait=backoff - 1 - i)) for i in range(1, backoff)]
    calls += [(first_hint, 1, dict(seq=seq + 1))]
    return calls


FEEDBACK_CASES = {
    "first call: no outcome yet": feedback(1, 4, 32, state(), [(hint(), 1, dict(seq=1))]),
    "first call, host guess": feedback(0, 4, 32, state(backoff=8), [(hint(word0(0, 3)), 1, dict(seq=1))]),
    "the outcome has not arrived": feedback(1, 4, 32, state(seq=5, acted=4, geo=2, backoff=8),
                                            [(hint(word0(4, 0), bits(20), 4, 16), 1, dict(seq=6))]),
    "accepted with tile 3": feedback(1, 4, 32, state(seq=5, acted=4, refused=1),
                                     [(hint(word0(5, 3)), 1, dict(seq=6, acted=5, geo=3, refused=0))]),
    "refused with back-off 0: the next call attempts": feedback(1, 4, 32, state(seq=5, acted=4, geo=3),
                                                                [(hint(word0(5, 0)), 1, dict(seq=6, acted=5, refused=1)),
                                                                 (hint(word0(5, 0)), 1, dict(seq=7))]),
    "refused with back-off 8": feedback(1, 4, 32, state(seq=5, acted=4, geo=3, backoff=8),
                                        backoff_calls(5, 8, hint(word0(5, 0)), dict(acted=5, refused=1))),
    "refused with back-off 8, host guess, bits unknown": feedback(0, 4, 32, state(seq=5, acted=4, backoff=8),
                                                                  backoff_calls(5, 8, hint(word0(5, 0), bits(20), 4), dict(acted=5, refused=1))),
    "an outcome that arrives while the object waits is not looked at": feedback(
        1, 4, 32, state(seq=5, acted=5, wait=2, refused=1, backoff=8),
        [(hint(word0(5, 3)), 0, dict(wait=1)), (hint(word0(5, 3)), 0, dict(wait=0)), (hint(word0(5, 3)), 1, dict(seq=6, geo=3, refused=0))]),
    # device_top: the sample missed a varying bit -- the exact top bit becomes the floor, and no back-off even with back-off 8;
    # a later outcome whose exact top bit lies below the floor clears it
    "device_top: refused with exact > used": feedback(1, 4, 32, state(seq=5, acted=4, backoff=8),
                                                      [(hint(word0(5, 0), bits(28), 5, 24), 1, dict(seq=6, acted=5, refused=1, floor=28)),
                                                       (hint(word0(6, 2), bits(20), 6, 28), 1, dict(seq=7, acted=6, refused=0, geo=2, floor=0))]),
    "device_top: refused for its runs (exact <= used): back-off": feedback(
        1, 4, 32, state(seq=5, acted=4, floor=28, backoff=3), backoff_calls(5, 3, hint(word0(5, 0), bits(28), 5, 28), dict(acted=5, refused=1))),
    "device_top: accepted with exact > used is no miss": feedback(1, 4, 32, state(seq=5, acted=4, backoff=8),
                                                                  [(hint(word0(5, 1), bits(28), 5, 24), 1, dict(seq=6, acted=5, geo=1))]),
    "device_top: bits of another attempt are not used": feedback(1, 4, 32, state(seq=5, acted=4, floor=28),
                                                                 [(hint(word0(5, 2), bits(20), 4, 28), 1, dict(seq=6, acted=5, geo=2))]),
    # the host's guess: 20 varying bits -- the assumption changed, so no back-off; refused again under it: back-off
    "host guess: 20 varying bits, then refused again": feedback(
        0, 4, 32, state(seq=5, acted=4, backoff=8),
        [(hint(word0(5, 0), bits(20), 5), 1, dict(seq=6, acted=5, refused=1, top=20))]
        + backoff_calls(6, 8, hint(word0(6, 0), bits(20), 6), dict(acted=6))),
    "host guess: accepted under the same assumption": feedback(0, 4, 32, state(seq=5, acted=4, top=20, backoff=8),
                                                               [(hint(word0(5, 4), bits(20), 5), 1, dict(seq=6, acted=5, geo=4))]),
    "host guess, 64-bit keys: 45 varying bits give 48": feedback(0, 8, 64, state(seq=1), [(hint(word0(1, 1), bits(45), 1), 1, dict(seq=2, acted=1, geo=1, top=48))]),
    "host guess, 64-bit keys: 37 varying bits give 40": feedback(0, 8, 64, state(seq=1), [(hint(word0(1, 1), bits(37), 1), 1, dict(seq=2, acted=1, geo=1, top=40))]),
    "host guess, 64-bit keys: 40 and 52 stay": feedback(0, 8, 64, state(seq=1),
                                                        [(hint(word0(1, 1), bits(40), 1), 1, dict(seq=2, acted=1, geo=1, top=40)),
                                                         (hint(word0(2, 1), bits(52), 2), 1, dict(seq=3, acted=2, top=52))]),
    "host guess, 32-bit keys are not rounded": feedback(0, 4, 32, state(seq=1), [(hint(word0(1, 1), bits(27), 1), 1, dict(seq=2, acted=1, geo=1, top=27))]),
    "host guess: no varying bit gives 16": feedback(0, 4, 32, state(seq=1), [(hint(word0(1, 1), bits(0), 1), 1, dict(seq=2, acted=1, geo=1, top=16))]),
    "host guess: few varying bits give 16": feedback(0, 4, 32, state(seq=1, top=24), [(hint(word0(1, 1), bits(9), 1), 1, dict(seq=2, acted=1, geo=1, top=16))]),
    "host guess: clamped to end_bit": feedback(0, 4, 32, state(seq=1, top=20), [(hint(word0(1, 1), bits(40), 1), 1, dict(seq=2, acted=1, geo=1, top=32))]),
    "wrap": feedback(1, 4, 32, state(seq=0x0FFFFFFF, acted=0x0FFFFFFE), [(hint(word0(0x0FFFFFFE, 2)), 1, dict(seq=1))]),
    "wrap behind an outcome": feedback(1, 4, 32, state(seq=0x0FFFFFFF, acted=0x0FFFFFFE),
                                       [(hint(word0(0x0FFFFFFF, 2)), 1, dict(seq=1, acted=0x0FFFFFFF, geo=2)),
                                        (hint(word0(0x0FFFFFFF, 2)), 1, dict(seq=2))]),
    "no hint words: every call attempts": feedback(1, 4, 32, state(seq=5, acted=4, wait=3, backoff=8), [(None, 1, dict(seq=6)), (None, 1, dict(seq=7))]),
}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sort_call_plan")
    src = tmp / "sort_call_plan.cpp"
    src.write_text(PROGRAM)
    lines = [str(len(PASS_CASES) + len(FEEDBACK_CASES))]
    for args, _ in PASS_CASES.values():
        lines.append(" ".join(str(x) for x in args))
    for device_top, key_bytes, end_bit, start, calls in FEEDBACK_CASES.values():
        lines.append(" ".join(str(x) for x in (1, device_top, key_bytes, end_bit, *(start[f] for f in FIELDS), len(calls))))
        for words, _, _ in calls:
            lines.append(" ".join(str(x) for x in ((1, *words) if words is not None else (0, 0, 0, 0, 0, 0))))
    infile = tmp / "cases.txt"
    infile.write_text("\n".join(lines) + "\n")
    return tmp, src, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    """The program's output lines: one per pass list, one per call of a feedback case."""
    tmp, src, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "sort_call_plan", [])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = [[int(x) for x in line.split()] for line in open(outfile).read().splitlines()]
    assert len(rows) == len(PASS_CASES) + sum(len(c[4]) for c in FEEDBACK_CASES.values())
    return rows


@pytest.mark.parametrize("name", list(PASS_CASES))
def test_pass_list(results, name):
    _, want = PASS_CASES[name]
    row = results[list(PASS_CASES).index(name)]
    assert row[:2] == [1, len(want)], name
    got = [tuple(row[2 + 4 * p:6 + 4 * p]) for p in range(row[1])]
    assert got == want, name


@pytest.mark.parametrize("name", list(FEEDBACK_CASES))
def test_attempt_feedback(results, name):
    names = list(FEEDBACK_CASES)
    first = len(PASS_CASES) + sum(len(FEEDBACK_CASES[n][4]) for n in names[:names.index(name)])
    _, _, _, start, calls = FEEDBACK_CASES[name]
    now = dict(start)
    for i, (_, attempts, changes) in enumerate(calls):
        assert set(changes) <= set(FIELDS)
        now.update(changes)
        row = results[first + i]
        assert row[0] == attempts, (name, i)
        assert dict(zip(FIELDS, row[1:])) == now, (name, i)


def test_the_sanitized_stand_alone_program_runs_clean(setup, results):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly; it
    writes what the plain build wrote."""
    tmp, src, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "sort_call_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert [[int(x) for x in line.split()] for line in open(outfile).read().splitlines()] == results


def test_the_list_is_as_long_as_the_device_side_plan():
    """The plain header cannot include the kernels' header: its capacity is a constant of its own, held to kPlanMaxPasses by a
    static_assert in the sort's translation unit.  Both stay there."""
    import re
    own = int(re.search(r"constexpr uint32_t kSortCallMaxPasses = (\d+);", open(os.path.join(CSRC, "sort_call_plan.hpp")).read()).group(1))
    plan = int(re.search(r"constexpr int kPlanMaxPasses = (\d+);", open(os.path.join(CSRC, "radix_sort_kernels.hpp")).read()).group(1))
    assert own == plan == 32
    assert "static_assert(kSortCallMaxPasses == (uint32_t) kPlanMaxPasses" in open(os.path.join(CSRC, "glu_hip.hip")).read()
