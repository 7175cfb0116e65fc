"""CPU test of the tiles that key runs and select share (csrc/tile_span.hpp): which elements of which 16-byte-aligned base an array
is, how many tiles it takes from there, and what the plan says for its count.  The header is plain C++: a host program prints the
span and the plan over a grid of element sizes, misalignments and counts, and the rules stated in the header are recomputed here.
No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

THREADS, SCAN_ROUND = 256, 4096
SHAPES = [(1, 1), (4, 4), (8, 4)]  # (element bytes, packs per thread): select's byte stencil; 4-byte keys and stencils; 8-byte ones
ADDRESS = 0x7F0000001000  # a 16-byte boundary; nothing is read through it


def vec(nbytes):
    return 16 // nbytes


def tile(nbytes, packs):
    return THREADS * packs * vec(nbytes)


def counts(nbytes, packs):
    return sorted({0, 1, vec(nbytes) - 1, vec(nbytes), (1 << 32) - 1}
                  | {tile(nbytes, packs) * m + d for m in (1, 2, 4096, 4097) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(element bytes, packs, misalignment in bytes, count): (base, lo, hi, tiles, plan tile, plan tiles, plan rounds)} as the
    header computes them, and {(element bytes, packs): (VEC, TILE)} of TileCfg."""
    tmp = tmp_path_factory.mktemp("tile_span")
    body = []
    for nbytes, packs in SHAPES:
        t = "uint%d_t" % (8 * nbytes)
        body.append('    printf("cfg %d %d %%u %%u\\n", TileCfg<%d, %d>::VEC, TileCfg<%d, %d>::TILE);' % (nbytes, packs, nbytes, packs, nbytes, packs))
        body.append("    for (unsigned long long mis = 0; mis < 16; mis += %d)" % nbytes)
        body.append("        for (unsigned long long count : {%s})" % ", ".join("%dull" % c for c in counts(nbytes, packs)))
        body.append("        {")
        body.append("            const TileSpan<%s> s = tile_span<%s, %d>((const void*) (uintptr_t) (%dull + mis), count);" % (t, t, packs, ADDRESS))
        body.append("            const TilePlan p = tile_plan(count, %d, %d);" % (nbytes, packs))
        body.append('            printf("span %d %d %%llu %%llu %%llu %%llu %%llu %%u %%u %%u %%u\\n", mis, count, (unsigned long long) (uintptr_t) s.base,'
                    % (nbytes, packs))
        body.append("                   (unsigned long long) s.lo, (unsigned long long) s.hi, s.tiles, p.tile, p.tiles, p.scan_rounds);")
        body.append("        }")
    src = tmp / "span.cpp"
    src.write_text('#include <cstdio>\n'
                   '#include <initializer_list>\n'
                   '#include "tile_span.hpp"\n'
                   "using namespace glu_hip;\n"
                   "int main()\n"
                   "{\n"
                   '    static_assert(sizeof(void*) == 8 && sizeof(unsigned long long) == 8, "counts and addresses are 64 bits wide");\n'
                   '    printf("consts %u %u %u %u\\n", kTileLanes, kTileThreads, kTileWaves, kTileScanRound);\n'
                   + "\n".join(body) + "\n"
                   "    return 0;\n"
                   "}\n")
    exe = tmp / "span"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    spans, cfgs, consts = {}, {}, None
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "consts":
            consts = tuple(v)
        elif kind == "cfg":
            cfgs[v[0], v[1]] = (v[2], v[3])
        else:
            spans[tuple(v[:4])] = tuple(v[4:])
    return spans, cfgs, consts


def test_the_geometry_is_256_threads_of_16_byte_packs(printed):
    _, cfgs, consts = printed
    assert consts == (64, THREADS, THREADS // 64, SCAN_ROUND)
    assert cfgs == {(nbytes, packs): (vec(nbytes), tile(nbytes, packs)) for nbytes, packs in SHAPES}


def test_every_span_and_plan_follows_the_rules_of_the_header(printed):
    spans, _, _ = printed
    assert len(spans) == sum(16 // nbytes * len(counts(nbytes, packs)) for nbytes, packs in SHAPES)
    for (nbytes, packs, mis, count), (base, lo, hi, tiles, plan_tile, plan_tiles, plan_rounds) in spans.items():
        case = (nbytes, packs, mis, count)
        first, t = ADDRESS + mis, tile(nbytes, packs)
        assert base % 16 == 0 and base <= first and base + lo * nbytes == first, case
        assert lo < vec(nbytes) and lo == mis // nbytes, case
        assert hi - lo == count, case
        assert tiles == (-(-hi // t) if count else 0), case
        assert plan_tile == t and plan_tiles == -(-count // t), case
        assert plan_tiles <= tiles <= plan_tiles + 1, case  # (what the reserve of the tile counts relies on)
        assert plan_rounds == -(-plan_tiles // SCAN_ROUND), case
        assert tiles < 1 << 32 and hi < (1 << 32) + vec(nbytes), case
    # (a misaligned base does add a tile somewhere on the grid, and a count of 2^32 - 1 is on it)
    assert any(v[3] == v[5] + 1 for v in spans.values())
    assert all((nbytes, packs, 0, (1 << 32) - 1) in spans for nbytes, packs in SHAPES)


def test_the_bindings_plans_are_the_headers(built, printed):
    """glu_key_runs_plan and glu_select_plan answer through tile_plan: key runs with four packs per thread, select with four, or one
    for the byte stencil."""
    spans, _, _ = printed
    assert built.plan_key_runs(1, 32)[0] == tile(4, 4) and built.plan_key_runs(1, 64)[0] == tile(8, 4)
    assert built.plan_select(1, built.SelectStencil_Byte)[0] == tile(1, 1)
    for stencil_type in (built.SelectStencil_Float, built.SelectStencil_Int, built.SelectStencil_Uint):
        assert built.plan_select(1, stencil_type)[0] == tile(4, 4)
    assert built.plan_select(1, built.SelectStencil_Double)[0] == tile(8, 4)
    for (nbytes, packs, mis, count), v in spans.items():
        if mis:
            continue
        if nbytes == 1:
            assert built.plan_select(count, built.SelectStencil_Byte) == v[4:], count
        else:
            assert built.plan_key_runs(count, 8 * nbytes) == v[4:], (nbytes, count)
            assert built.plan_select(count, built.SelectStencil_Uint if nbytes == 4 else built.SelectStencil_Double) == v[4:], (nbytes, count)
