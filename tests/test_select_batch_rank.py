"""CPU test of the arithmetic of the batched select (csrc/select_batch_rank.hpp): where the flag of an element lies in the words the
count kernel stores, and the rank of an arbitrary position from a scanned tile count, a wave sum and one wave's words under a mask.
The header is plain C++: a host program draws random flag arrays, builds the flag words, the wave sums and the scanned tile counts
in the kernel's layout by walking (tile, wave, pack, lane, element) forwards as the count kernel does, and holds select_batch_rank(p)
against a running sum at EVERY position p = 0 .. count -- for the three stencil widths, at every shift of the array off a 16-byte
boundary, at one wave part, one tile and three tiles + 17, each +- 1, at several densities.  Every index into the three arrays is
checked against its bound.  The same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a
stand-alone executable with identical output.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "select_batch_rank.hpp"
using namespace glu_hip;

static unsigned long long violations = 0, positions = 0;
static uint64_t state = 88172645463325252ull;
static uint32_t draw()
{
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (uint32_t) (state >> 16);
}

// `count` elements from element `lo` of an aligned base; one in `one_in` is flagged (0: all, 0xFFFFFFFF: none)
template<uint32_t ELEM_BYTES, uint32_t PACKS>
static void one_case(uint32_t lo, uint32_t count, uint32_t one_in)
{
    using C = SelectBatchCfg<ELEM_BYTES, PACKS>;
    std::vector<uint8_t> flag(count);
    for (uint32_t i = 0; i < count; i++) flag[i] = one_in == 0 ? 1 : one_in == 0xFFFFFFFFu ? 0 : draw() % one_in == 0;
    const uint64_t hi = (uint64_t) lo + count;
    const uint32_t tiles = count ? tile_plan(hi, ELEM_BYTES, PACKS).tiles : 0;
    const SelectBatchScratch at = select_batch_scratch(count, ELEM_BYTES, PACKS);
    if (count && ((size_t) tiles + 1 > (at.below_at - at.counts_at) / 4 || (size_t) tiles * 16 > at.flags_at - at.below_at ||
                  (size_t) tiles * C::TILE_FLAG_BYTES > at.bytes - at.flags_at || at.below_at % 16 || at.flags_at % 16))
        violations++; // (the scratch of a prepared call holds what a call at any shift stores)
    // the count kernel, lane by lane
    std::vector<uint32_t> tile_scan(tiles + 1, 0), wave_below(4 * (size_t) tiles, 0);
    std::vector<uint64_t> words((size_t) tiles * C::TILE_WORDS, 0);
    uint8_t* lane_flags = reinterpret_cast<uint8_t*>(words.data());
    for (uint32_t t = 0; t < tiles; t++)
    {
        uint32_t in_tile = 0;
        for (uint32_t w = 0; w < kTileWaves; w++)
        {
            wave_below[4 * (size_t) t + w] = in_tile;
            for (uint32_t lane = 0; lane < kTileLanes; lane++)
            {
                uint32_t f = 0;
                for (uint32_t g = 0; g < C::PACKS; g++)
                    for (uint32_t k = 0; k < C::VEC; k++)
                    {
                        const uint64_t v = (uint64_t) t * C::TILE + w * C::WAVE_ELEMS + lane * C::VEC + g * C::PACK_STRIDE + k;
                        if (v >= lo && v < hi && flag[v - lo]) f |= 1u << (g * C::VEC + k), in_tile++;
                    }
                const size_t thread = (size_t) t * kTileThreads + w * kTileLanes + lane;
                for (uint32_t b = 0; b < C::LANE_BITS / 8; b++) lane_flags[thread * (C::LANE_BITS / 8) + b] = (uint8_t) (f >> (8 * b)); // (little-endian)
            }
        }
        tile_scan[t + 1] = tile_scan[t] + in_tile;
    }
    // every position against the running sum
    unsigned long long mismatches = 0;
    uint32_t running = 0;
    for (uint32_t p = 0; p <= count && tiles; p++)
    {
        const uint32_t got = select_batch_rank<C>((uint64_t) lo + p, tiles, tile_scan.data(), wave_below.data(), [&](size_t i) {
            if (i >= words.size())
            {
                violations++;
                return (uint64_t) 0;
            }
            return words[i];
        });
        if (got != running) mismatches++;
        if (p < count) running += flag[p];
        positions++;
    }
    printf("%u %u %u %u %u %llu\n", ELEM_BYTES, lo, count, one_in, running, mismatches);
}

template<uint32_t ELEM_BYTES, uint32_t PACKS>
static void width()
{
    using C = SelectBatchCfg<ELEM_BYTES, PACKS>;
    static_assert(C::TILE_FLAG_BYTES * 8 == C::TILE && C::WAVE_WORDS * 64 == C::WAVE_ELEMS, "one bit per element");
    const uint32_t sizes[] = {1, 2, C::VEC, C::PACK_STRIDE - 1, C::PACK_STRIDE, C::PACK_STRIDE + 1, C::WAVE_ELEMS - 1, C::WAVE_ELEMS, C::WAVE_ELEMS + 1,
                              C::TILE - 1, C::TILE, C::TILE + 1, 3 * C::TILE + 17};
    const uint32_t densities[] = {2, 0, 0xFFFFFFFFu, 13, 1000};
    for (uint32_t lo = 0; lo < C::VEC; lo++) // every shift the element size allows
        for (uint32_t count : sizes)
            for (uint32_t d = 0; d < 5; d++)
            {
                if (d >= 3 && lo != 0 && lo != C::VEC - 1) continue; // (the sparse densities at the first and the last shift)
                one_case<ELEM_BYTES, PACKS>(lo, count, densities[d]);
            }
    one_case<ELEM_BYTES, PACKS>(0, 0, 2);
}

int main()
{
    width<4, 4>();
    width<8, 4>();
    width<1, 1>();
    printf("positions %llu violations %llu\n", positions, violations);
    return violations ? 1 : 0;
}
"""


def build_and_run(tmp, name, flags):
    src, exe = tmp / "select_batch_rank.cpp", tmp / name
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("select_batch_rank"), "select_batch_rank", [])


def test_the_rank_of_every_position_is_the_running_sum(plain):
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr
    lines = plain.stdout.splitlines()
    rows = [tuple(int(x) for x in line.split()) for line in lines[:-1]]
    assert lines[-1].startswith("positions ") and lines[-1].endswith(" violations 0")
    assert int(lines[-1].split()[1]) > 10 ** 6
    tiles = {4: 4096, 8: 2048, 1: 4096}
    for elem_bytes, tile in tiles.items():
        mine = [r for r in rows if r[0] == elem_bytes]
        vec, wave = 16 // elem_bytes, tile // 4
        assert {r[1] for r in mine} == set(range(vec))  # every shift off a 16-byte boundary
        for lo in range(vec):
            sizes = {r[2] for r in mine if r[1] == lo}
            assert {wave - 1, wave, wave + 1, tile - 1, tile, tile + 1, 3 * tile + 17} <= sizes, (elem_bytes, lo)
        assert any(r[2] == 0 for r in mine)
    assert all(r[5] == 0 for r in rows), [r for r in rows if r[5]][:10]
    # the flags were what the densities say: all, none, about half
    assert all(r[4] == r[2] for r in rows if r[3] == 0) and all(r[4] == 0 for r in rows if r[3] == 0xFFFFFFFF)
    assert all(0.4 * r[2] < r[4] < 0.6 * r[2] for r in rows if r[3] == 2 and r[2] > 1000)


def test_the_same_program_is_clean_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    p = build_and_run(tmp_path, "select_batch_rank_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert p.returncode == 0 and p.stderr == "", p.stderr[-3000:]
    assert p.stdout == plain.stdout


def test_the_tiles_the_header_states_are_the_plans(built):
    for stencil_type, elem_bytes, packs in ((built.SelectStencil_Uint, 4, 4), (built.SelectStencil_Double, 8, 4), (built.SelectStencil_Byte, 1, 1)):
        tile = built.plan_select_batch(1, 1, stencil_type)[0]
        assert tile == 256 * packs * (16 // elem_bytes) == built.plan_select(1, stencil_type)[0]
