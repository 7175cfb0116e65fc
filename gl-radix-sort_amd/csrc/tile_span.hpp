// tile_span.hpp -- the tiles of key runs and select (tile_compact_kernels.hpp): how many elements a tile holds, which elements of
// which aligned base an array is, how many tiles and rounds of the count scan a call takes.  Once for both operators, and plain
// C++: tests/test_tile_span.py includes this header with a host compiler.
#pragma once

#include <cstddef>
#include <cstdint>

namespace glu_hip
{
// (tile_compact_kernels.hpp asserts that these are the wave, the workgroup of the batched scan and its tile of 4-byte counts)
constexpr uint32_t kTileLanes = 64, kTileThreads = 256, kTileWaves = kTileThreads / kTileLanes;
constexpr uint32_t kTileScanRound = 4096; // counts per round of the count scan

// A tile: 256 threads x PACKS packs of 16 bytes, wave-major, then pack, then lane, then the elements of a pack, so that the order
// of (wave, pack, lane, element) is the order of the elements.
constexpr uint32_t tile_elems(uint32_t elem_bytes, uint32_t packs) { return kTileThreads * packs * (16 / elem_bytes); }

template<uint32_t ELEM_BYTES, uint32_t PACKS_>
struct TileCfg
{
    static constexpr uint32_t VEC = 16 / ELEM_BYTES;            // elements of a pack
    static constexpr uint32_t PACKS = PACKS_;                   // packs per thread and tile
    static constexpr uint32_t PACK_STRIDE = kTileLanes * VEC;   // from a lane's pack g to its pack g + 1
    static constexpr uint32_t WAVE_ELEMS = PACKS * PACK_STRIDE; // elements of a wave
    static constexpr uint32_t TILE = tile_elems(ELEM_BYTES, PACKS);
    static_assert(TILE == kTileWaves * WAVE_ELEMS, "a tile is its waves");
    static_assert(PACKS * VEC <= 32, "a lane's flags are the bits of one word");
};

// elements per tile, tiles of `count` elements from an aligned base, rounds of the count scan
struct TilePlan
{
    uint32_t tile, tiles, scan_rounds;
};
inline TilePlan tile_plan(uint64_t count, uint32_t elem_bytes, uint32_t packs)
{
    TilePlan p;
    p.tile = tile_elems(elem_bytes, packs);
    p.tiles = (uint32_t) ((count + p.tile - 1) / p.tile);
    p.scan_rounds = (p.tiles + kTileScanRound - 1) / kTileScanRound;
    return p;
}

// An array as the streaming kernels see it.  `base` is the 16-byte boundary at or below the array; the array is the elements
// [lo, hi) of it (lo < VEC), and tiles are counted from `base`: every pack is aligned.  A base below the array moves the elements up
// to a pack's length into the first tile, which can add a tile behind the last: one more than the plan's, never two.
template<typename T>
struct TileSpan
{
    const T* base;
    uint64_t lo, hi;
    uint32_t tiles;
};

template<typename T, uint32_t PACKS>
inline TileSpan<T> tile_span(const void* first, uint64_t count)
{
    TileSpan<T> s;
    s.lo = ((uintptr_t) first & 15u) / sizeof(T);
    s.hi = s.lo + count;
    s.base = (const T*) first - s.lo;
    s.tiles = count ? tile_plan(s.hi, (uint32_t) sizeof(T), PACKS).tiles : 0u;
    return s;
}

} // namespace glu_hip
