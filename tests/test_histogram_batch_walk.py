"""CPU test of what decides which memory the batched histogram touches (csrc/histogram_batch_walk.hpp over batch_lists.hpp): the
clamp of a segment, the class of a length, the packs and masks of a span, the chunks of a long segment and its run of slots, the row
index.  The headers are plain C++: a host program performs whole calls through their functions alone, as histogram_batch_kernels.hpp
does -- binning in a shuffled arrival order into the lists of batch_lists_layout, then the wave list, the block list, the chunk list and
the long list (or, for equal partitions, the class the plan picks) -- and reports how often every sample was read, how often every row
was written, the class of every segment and whether any index left its array: a sample outside [0, total), a row outside the
num_segments * bins counts, a slot outside the reserved scratch, a list entry outside its list.  Well-formed offsets are held against
numpy's restatement of the classes and against "every sample of a segment exactly once"; shuffled, decreasing and out-of-range offsets
only against the promise that every index stays inside.  The same program, built with the address and undefined-behaviour
sanitizers, runs the same cases as a stand-alone executable.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "histogram_batch_walk.hpp"
using namespace glu_hip;

static unsigned long long violations = 0;
static FILE* in;
static FILE* out;

template<typename T>
static std::vector<T> get(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) exit(3);
    return v;
}
template<typename T>
static void put(const std::vector<T>& v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), out) != v.size()) exit(4);
}
static void require(bool ok)
{
    if (!ok) violations++;
}

struct Header
{
    uint32_t num_segments, total, bins, key_bytes, with_offsets, count, misalign, seed;
};

struct Call
{
    Header h;
    std::vector<uint32_t> offsets;
    std::vector<uint8_t> visited;  // per sample: how often it was read
    std::vector<uint8_t> written;  // per segment: how often its row was written
    std::vector<uint8_t> cls;      // per segment: 0 empty, 1 wave, 2 block, 3 long
    uint64_t slots;                // rows of the reserved scratch
};

template<typename T>
struct Walk
{
    Call& c;
    const T* samples; // sample 0 of the batch: `misalign` elements behind a 16-byte boundary of a larger allocation

    void segment(uint32_t seg, uint64_t& begin, uint64_t& len) const
    {
        require(seg < c.h.num_segments);
        hist_batch_segment(c.h.with_offsets != 0, [&](uint32_t i) {
            require(i < c.offsets.size());
            return i < c.offsets.size() ? c.offsets[i] : 0u;
        }, c.h.count, c.h.total, seg, begin, len);
        require(begin + len <= c.h.total || len == 0);
    }
    // the packs a kernel reads of the samples [begin, begin + len): `stride` packs a round, every round whole (the packs behind the
    // span's last are masked), every element by tile_load_pack's rule: read iff lo <= v < hi
    void read(uint64_t begin, uint64_t len, uint32_t stride) const
    {
        constexpr uint32_t VEC = 16 / sizeof(T);
        const TileSpan<T> span = hist_batch_span(samples, begin, len);
        require(span.lo < VEC && ((uintptr_t) span.base & 15u) == 0);
        uint64_t seen = 0;
        for (uint64_t p0 = 0; p0 < span.tiles; p0 += stride)
            for (uint64_t p = p0; p < p0 + stride; p++)
                for (uint32_t k = 0; k < VEC; k++)
                {
                    const uint64_t v = p * VEC + k;
                    if (v < span.lo || v >= span.hi) continue;
                    const int64_t i = (span.base + v) - samples;
                    if (i < 0 || i >= (int64_t) c.h.total) violations++;
                    else if (c.visited[i] < 255) c.visited[i]++;
                    seen++;
                }
        require(seen == len);
    }
    void write_row(uint32_t seg) const
    {
        require(hist_batch_row(seg, c.h.bins) + c.h.bins <= (uint64_t) c.h.num_segments * c.h.bins);
        if (seg < c.written.size() && c.written[seg] < 255) c.written[seg]++;
    }
    void write_slot(uint64_t slot) const { require(hist_batch_row(slot, c.h.bins) + c.h.bins <= c.slots * c.h.bins); }

    void equal_partitions() const
    {
        const HistBatchPlan p = hist_batch_plan(c.h.count, c.h.bins, sizeof(T));
        const uint32_t S = c.h.num_segments;
        std::fill(c.cls.begin(), c.cls.end(), (uint8_t) p.path);
        c.slots = p.path == 3 ? (uint64_t) p.workgroups * S : 0;
        uint64_t begin, len;
        if (p.path == 0)
            for (uint32_t s = 0; s < S; s++) write_row(s);
        else if (p.path <= 2)
            for (uint32_t s = 0; s < S; s++)
            {
                segment(s, begin, len);
                read(begin, len, p.path == 1 ? 64u * kHistPacks : hist_threads(sizeof(T), HIST_EDGES) * kHistPacks);
                write_row(s);
            }
        else
        {
            for (uint64_t li = 0; li < c.slots; li++)
            {
                const uint32_t seg = (uint32_t) (li / p.workgroups), chunk = (uint32_t) (li % p.workgroups);
                segment(seg, begin, len);
                uint64_t at;
                uint32_t part;
                hist_batch_chunk_range(len, chunk, p.chunk, at, part);
                read(begin + at, part, hist_threads(sizeof(T), HIST_EVEN) * kHistPacks);
                write_slot(li);
            }
            for (uint32_t s = 0; s < S; s++) write_row(s);
        }
    }

    void device_offsets() const
    {
        const uint32_t S = c.h.num_segments;
        size_t words;
        const BatchListsLayout layout = batch_lists_layout(hist_batch_classes(c.h.bins, sizeof(T)), c.h.total, S, words);
        c.slots = hist_batch_slots(c.h.total, S, layout.limit[BATCH_LIST_BLOCK], layout.chunk);
        require(c.slots == layout.capacity[BATCH_LIST_CHUNKS]);
        require(c.slots * c.h.bins * 4 <= (uint64_t) c.h.total / 8 + 0); // the scratch of a batch stays at or below total / 8 bytes
        std::vector<uint32_t> lists(words, 0xA5A5A5A5u), filled(words, 0);
        uint64_t counts[BATCH_LISTS] = {0, 0, 0, 0, 0, 0}; // (counts[BATCH_LIST_CHUNKS]: the 64-bit counter of chunk slots)
        const auto store = [&](int list, uint64_t at, uint32_t entry_words, uint32_t a, uint32_t b) {
            const uint64_t w = layout.start[list] + at * entry_words;
            if (at >= layout.capacity[list] || w + entry_words > words)
            {
                violations++;
                return;
            }
            lists[w] = a;
            if (entry_words == 2) lists[w + 1] = b;
            filled[w]++;
        };
        // binning, in an arrival order of its own
        std::vector<uint32_t> order(S);
        for (uint32_t s = 0; s < S; s++) order[s] = s;
        std::mt19937 rng(c.h.seed);
        std::shuffle(order.begin(), order.end(), rng);
        uint64_t begin, len;
        for (uint32_t seg : order)
        {
            segment(seg, begin, len);
            const int cls = hist_batch_class(len, layout.limit[BATCH_LIST_SHORT4], layout.limit[BATCH_LIST_BLOCK]);
            c.cls[seg] = cls < 0 ? 0 : cls == BATCH_LIST_SHORT4 ? 1 : cls == BATCH_LIST_BLOCK ? 2 : 3;
            if (cls < 0) write_row(seg); // (the zeroing; not under accumulate)
            else if (cls != BATCH_LIST_LONG)
            {
                const uint64_t at = counts[cls]++;
                if (at < layout.capacity[cls]) store(cls, at, 1, seg, 0);
            }
            else
            {
                const uint32_t nchunks = hist_batch_chunks(len, layout.chunk);
                const uint64_t got = counts[BATCH_LIST_CHUNKS];
                counts[BATCH_LIST_CHUNKS] += nchunks;
                const uint32_t capacity = layout.capacity[BATCH_LIST_CHUNKS];
                const uint32_t slot = got < capacity ? (uint32_t) got : capacity;
                if (batch_chunk_run_fits(got, nchunks, capacity))
                {
                    const uint64_t at = counts[BATCH_LIST_LONG]++;
                    if (at < layout.capacity[BATCH_LIST_LONG]) store(BATCH_LIST_LONG, at, 2, seg, slot);
                }
                for (uint32_t k = 0; k < nchunks; k++)
                    if ((uint64_t) slot + k < capacity) store(BATCH_LIST_CHUNKS, slot + k, 2, seg, k);
            }
        }
        const auto length = [&](int list) { return (uint32_t) std::min<uint64_t>(counts[list], layout.capacity[list]); };
        const auto entry = [&](int list, uint64_t at, uint32_t entry_words, uint32_t word) {
            const uint64_t w = layout.start[list] + at * entry_words;
            require(w + entry_words <= words && filled[w] == 1); // every entry a kernel walks was written, once
            return w + word < words ? lists[w + word] : 0u;
        };
        require(length(BATCH_LIST_SHORT16) == 0 && length(BATCH_LIST_SHORT64) == 0);
        if (layout.limit[BATCH_LIST_SHORT4] == 0) require(length(BATCH_LIST_SHORT4) == 0);
        for (uint32_t li = 0; li < length(BATCH_LIST_SHORT4); li++) // the wave kernel
        {
            const uint32_t seg = entry(BATCH_LIST_SHORT4, li, 1, 0);
            segment(seg, begin, len);
            require(len <= hist_batch_wave_limit(c.h.bins, sizeof(T)) && c.h.bins <= kHistBatchWaveBins);
            read(begin, len, 64u * kHistPacks);
            write_row(seg);
        }
        for (uint32_t li = 0; li < length(BATCH_LIST_BLOCK); li++) // the block kernel
        {
            const uint32_t seg = entry(BATCH_LIST_BLOCK, li, 1, 0);
            segment(seg, begin, len);
            read(begin, len, hist_threads(sizeof(T), HIST_EVEN) * kHistPacks);
            write_row(seg);
        }
        for (uint32_t li = 0; li < length(BATCH_LIST_CHUNKS); li++) // the block kernel over the chunks
        {
            const uint32_t seg = entry(BATCH_LIST_CHUNKS, li, 2, 0), chunk = entry(BATCH_LIST_CHUNKS, li, 2, 1);
            segment(seg, begin, len);
            uint64_t at;
            uint32_t part;
            hist_batch_chunk_range(len, chunk, layout.chunk, at, part);
            require(at + part <= len);
            read(begin + at, part, hist_threads(sizeof(T), HIST_EDGES) * kHistPacks);
            write_slot(li);
        }
        for (uint32_t li = 0; li < length(BATCH_LIST_LONG); li++) // the sum kernel
        {
            const uint32_t seg = entry(BATCH_LIST_LONG, li, 2, 0), slot = entry(BATCH_LIST_LONG, li, 2, 1);
            segment(seg, begin, len);
            const uint32_t rows = hist_batch_chunks(len, layout.chunk);
            require((uint64_t) slot + rows <= length(BATCH_LIST_CHUNKS));
            for (uint32_t r = 0; r < rows && (uint64_t) slot + r < length(BATCH_LIST_CHUNKS); r++) // its rows are its own chunks, in order
                require(entry(BATCH_LIST_CHUNKS, slot + r, 2, 0) == seg && entry(BATCH_LIST_CHUNKS, slot + r, 2, 1) == r);
            write_row(seg);
        }
    }

    void run() const
    {
        if (c.h.num_segments == 0) return;
        if (c.h.with_offsets) device_offsets();
        else equal_partitions();
    }
};

template<typename T>
static void one_case(Call& c)
{
    constexpr uint32_t VEC = 16 / sizeof(T);
    std::vector<T> storage((size_t) c.h.total + 4 * VEC, (T) 7);
    size_t a0 = 0;
    while (((uintptr_t) (storage.data() + a0) & 15u) != 0) a0++;
    Walk<T> w{c, storage.data() + a0 + VEC + c.h.misalign % VEC};
    w.run();
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t cases = get<uint32_t>(1)[0];
    for (uint32_t i = 0; i < cases; i++)
    {
        const std::vector<uint32_t> w = get<uint32_t>(8);
        Call c;
        c.h = Header{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
        c.offsets = get<uint32_t>(c.h.with_offsets ? c.h.num_segments + 1 : 0);
        c.visited.assign(c.h.total, 0);
        c.written.assign(c.h.num_segments, 0);
        c.cls.assign(c.h.num_segments, 0);
        c.slots = 0;
        if (c.h.key_bytes == 4) one_case<uint32_t>(c);
        else one_case<uint64_t>(c);
        put(c.visited);
        put(c.written);
        put(c.cls);
        put(std::vector<uint64_t>{c.slots});
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    printf("cases %u violations %llu\n", cases, violations);
    return violations ? 1 : 0;
}
"""

WAVE_BYTES, WAVE_BINS, CHUNK_BYTES, PER_BIN = 8192, 2048, 1 << 19, 64  # restated from histogram_bins.hpp


def limits(bins, key_bytes):
    chunk = max(CHUNK_BYTES // key_bytes, PER_BIN * bins)
    return (WAVE_BYTES // key_bytes if bins <= WAVE_BINS else 0), chunk, chunk


def classes(lens, bins, key_bytes):
    wave, block, _ = limits(bins, key_bytes)
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens == 0, 0, np.where(lens <= wave, 1, np.where(lens <= block, 2, 3))).astype(np.uint8)


def offsets_from_lengths(lens, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) + first).astype(np.uint32)


class Case:
    def __init__(self, kind, bins, key_bytes, total, offsets=None, count=0, parts=0, misalign=0, seed=1):
        self.kind, self.bins, self.key_bytes, self.total, self.offsets = kind, bins, key_bytes, total, offsets
        self.count, self.misalign, self.seed = count, misalign, seed
        self.S = offsets.size - 1 if offsets is not None else parts

    def header(self):
        return np.array([self.S, self.total, self.bins, self.key_bytes, self.offsets is not None, self.count, self.misalign, self.seed],
                        dtype=np.uint32)


def make_cases():
    rng = np.random.default_rng(51)
    cases = []
    for key_bytes in (4, 8):
        vec = 16 // key_bytes
        for bins in (16, 2048, 2049, 8192):
            wave, block, chunk = limits(bins, key_bytes)
            w = wave if wave else 64
            pool = [0, 0, 0, 1, 2, vec - 1, vec, vec + 1, 63, 64, 65, 255 * vec, 256 * vec, 256 * vec + 1, w - 1, w, w + 1]
            for trial in range(3):
                lens = list(rng.choice(pool, 40)) + [block - 1, block, block + 1, 2 * chunk, 2 * chunk + 1, chunk + 5]
                lens = rng.permutation(lens)
                first, behind = ((0, 0), (3, 5), (1, 0))[trial]  # samples in front of and behind the batch belong to no segment
                offsets = offsets_from_lengths(lens, first)
                cases.append(Case("formed", bins, key_bytes, int(offsets[-1]) + behind, offsets, misalign=trial, seed=trial))
            # equal partitions: one count in each class, and none
            for count in (0, 1, w, w + 1, block, block + 1, 2 * chunk + 1):
                for misalign in (0, 1):
                    cases.append(Case("equal", bins, key_bytes, count * 5, count=count, parts=5, misalign=misalign))
        # malformed offsets
        wave, block, chunk = limits(16, key_bytes)
        lens = rng.permutation(list(rng.choice([0, 1, 5, 64, wave, wave + 1, 3000], 30)) + [block + 1, 2 * chunk + 1, chunk + 9, block])
        good = offsets_from_lengths(lens)
        total = int(good[-1])
        S = good.size - 1
        beyond = good.copy()
        beyond[S // 2:] += np.uint32(3 * chunk)
        wild = good.copy()
        wild[3], wild[-1] = np.uint32(0xFFFFFFFF), np.uint32(0xFFFFFFF0)
        last_below = good.copy()
        last_below[-1] = 1
        overlap = np.zeros(S + 1, dtype=np.uint32)
        overlap[1::2] = total  # every other segment is the whole array: far more chunks than the batch has
        for seed, bad in enumerate((rng.permutation(good).astype(np.uint32), good[::-1].copy(), beyond, wild, last_below, overlap,
                                    rng.integers(0, 2 ** 32, S + 1, dtype=np.uint32), rng.integers(0, total + 1, S + 1, dtype=np.uint32),
                                    np.full(S + 1, 0xFFFFFFFF, dtype=np.uint32))):
            cases.append(Case("malformed", 16, key_bytes, total, bad, misalign=seed % 3, seed=seed))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("histogram_batch_walk")
    src = tmp / "histogram_batch_walk.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for c in cases:
            f.write(c.header().tobytes())
            if c.offsets is not None:
                f.write(c.offsets.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "histogram_batch_walk", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for c in cases:
        out.append({"visited": take(np.uint8, c.total), "written": take(np.uint8, c.S), "cls": take(np.uint8, c.S),
                    "slots": int(take(np.uint64, 1)[0])})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p


def test_no_index_leaves_its_array_whatever_the_offsets_hold(setup, results):
    _, _, cases, _ = setup
    _, violations, p = results
    assert violations == 0 and p.returncode == 0 and p.stderr == ""
    assert p.stdout == "cases %d violations 0\n" % len(cases)
    assert sum(c.kind == "malformed" for c in cases) == 18


def test_every_sample_of_a_well_formed_segment_is_read_once_and_every_row_written_once(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if c.kind == "malformed":
            continue
        seen += 1
        name = (c.kind, c.bins, c.key_bytes, c.total, c.S, c.count, c.misalign)
        o = c.offsets.astype(np.int64) if c.offsets is not None else np.arange(c.S + 1, dtype=np.int64) * c.count
        want = np.zeros(c.total, dtype=np.uint8)
        want[o[0]:o[-1]] = 1
        assert (r["visited"] == want).all(), name
        assert (r["written"] == 1).all(), name
    assert seen == 2 * 4 * (3 + 14)


def test_numpy_restates_the_classes_and_the_reserved_slots(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    met = set()
    for c, r in zip(cases, out):
        if c.kind == "malformed":
            continue
        lens = np.diff(c.offsets.astype(np.int64)) if c.offsets is not None else np.full(c.S, c.count)
        want = classes(lens, c.bins, c.key_bytes)
        assert (r["cls"] == want).all(), (c.kind, c.bins, c.key_bytes)
        met |= {(c.bins > WAVE_BINS, int(k)) for k in want}
        _, _, chunk = limits(c.bins, c.key_bytes)
        if c.offsets is not None:
            slots = c.total // chunk + min(c.S, c.total // (chunk + 1))
            assert r["slots"] == slots and slots * c.bins * 4 <= c.total // 8
        else:
            assert r["slots"] == (-(-c.count // chunk) * c.S if want[0] == 3 else 0)
    assert met == {(False, 0), (False, 1), (False, 2), (False, 3), (True, 0), (True, 2), (True, 3)}  # no wave class beyond 2048 bins


def test_malformed_offsets_read_inside_the_samples_and_write_rows_at_most_once(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if c.kind != "malformed":
            continue
        seen += 1
        assert (r["written"] <= 1).all()
        o = c.offsets.astype(np.int64)
        formed = (o[:-1] <= o[1:]) & (o[1:] <= c.total)
        assert (r["cls"][~formed] == 0).all() and (r["written"][~formed] == 1).all()  # empty to every kernel: zeroed
        lens = np.where(formed, o[1:] - o[:-1], 0)
        assert (r["cls"] == classes(lens, c.bins, c.key_bytes)).all()
        if int(lens.sum()) <= c.total:  # the segments fit the array together: no list can overflow, every row is written
            assert (r["written"] == 1).all()
    assert seen == 18


def test_the_sanitized_stand_alone_program_runs_clean(setup, results):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly; it
    prints the same line and leaves stderr empty."""
    tmp, src, _, infile = setup
    _, _, plain = results
    p, outfile = build_and_run(tmp, src, infile, "histogram_batch_walk_san",
                               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert p.stderr == "" and p.stdout == plain.stdout
    assert open(outfile, "rb").read() == open(tmp / "histogram_batch_walk.out", "rb").read()
