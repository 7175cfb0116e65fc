"""GPU tests of every operator on long-lived objects over random call sequences (sequence_cases.py draws them and holds the numpy
answers).  One set of objects per sequence, forty calls in a drawn order on one stream: small after large, 4-byte after 8-byte keys,
other optional outputs and options than the call before, so that whatever a call leaves in the object's device-resident scratch
(counters, segment lists, tile counts, a remembered index, candidate arrays) meets a call it was not left for.  After every call the
stream is synchronised and every allocation the call was given, guards included, is compared byte for byte with numpy; what the
object reports about the call is compared with the host-only plan functions.  The first difference ends the sequence with the unit,
the seed, the index of the step and its scalar arguments."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import sequence_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# The child of the threads test took 2.1 s and 2.5 s in its first two runs on an MI355X (the import of torch and the creation of the
# device context included); the limit is twenty-four times the longer one, so that only a child that hangs meets it.
THREADS_CHILD_TIMEOUT = 60


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


@pytest.fixture(scope="module")
def drawn(built):
    """The steps of every committed sequence, drawn once and shared; no test changes them."""
    cache = {}

    def get(unit, seed):
        if (unit, seed) not in cache:
            cache[unit, seed] = sc.sequence(unit, seed)
        return cache[unit, seed]

    return get


@pytest.mark.parametrize("mode", ["prepared", "unprepared"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("unit", sc.UNITS)
def test_sequence(G, drawn, unit, which, mode):
    sc.run_sequence(G, drawn(unit, sc.SEEDS[unit][which]), prepared=mode == "prepared")


@pytest.mark.parametrize("unit", ["TopK", "Histogram", "SetOps"])
def test_twice_the_same_sequence_gives_the_same_bits(G, drawn, unit):
    """The units with arrival-order hazards on the device (the append of top-k's candidates and of its binning kernel, histogram's
    atomics on the counts, the scanned tile counts of the set operations): a second fresh set of objects, the same steps, the same
    bytes in every allocation of every step."""
    steps = drawn(unit, sc.SEEDS[unit][0])
    if unit == "Histogram":
        assert sum(sc.expected_diag(s)["last"][0] == sc.GLOBAL for s in steps) >= 2, "the sequence does not reach the atomic path"
    first = sc.run_sequence(G, steps, prepared=False)
    second = sc.run_sequence(G, steps, prepared=False)
    for step, a, b in zip(steps, first, second):
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), (sc.scalars(step), name)


def test_distinct_handles_on_distinct_host_threads():
    """The header's contract for threads: distinct handles may be used from distinct host threads.  A fresh process, so that the
    device is opened and every kernel's one-time setup is made for the first time with four threads arriving at once; each thread
    has its own objects (RadixSort batched, TopK, Merge, Reduce), its own stream and the first twelve steps of its unit's sequence."""
    begin = time.time()
    p = subprocess.run([sys.executable, os.path.join(HERE, "sequence_cases.py"), "threads"], capture_output=True, text=True,
                       timeout=THREADS_CHILD_TIMEOUT)
    print("the child took %.1f s" % (time.time() - begin))
    print(p.stdout[-4000:])
    print(p.stderr[-4000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("12 steps agree") == 4, p.stdout[-2000:]
