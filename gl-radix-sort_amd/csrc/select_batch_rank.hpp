// select_batch_rank.hpp -- the arithmetic of the BATCHED SELECT (select_batch_kernels.hpp, glu_select.hip) in plain C++: where the
// flags of an element lie in the scratch the count kernel leaves, and the rank of an arbitrary position from them -- the number of
// selected elements in front of it.  The offsets kernel includes this header, and tests/test_select_batch_rank.py includes it with
// a host compiler, builds the flag words the way the count kernel stores them and holds select_batch_rank against a running sum at
// every position: what holds there (every index inside its array, the rank at every position up to the end) holds on the device.
//
// The count kernel keeps, per tile t of the stencil (tile_span.hpp: wave-major, then pack, then lane, then the elements of a pack):
//   tile_scan[t]        the selected elements of the tiles in front of t (the count scan's output; entry `tiles` is the total)
//   wave_below[4t + w]  the selected elements of tile t in front of its wave w
//   the flag words      lane l of wave w holds PACKS * VEC elements, and bit g * VEC + k of its flag word is element k of its pack
//                       g: one bit per element, 8 or 16 bits per lane, the lanes of a wave side by side in lane order.  As 64-bit
//                       words a wave is kTileLanes * LANE_BITS / 64 of them (8 or 16: 64 or 128 bytes, one cache line).
// The rank of a position is then one count, one wave sum and the popcounts of ONE wave's words under a mask, whatever the data hold.
#pragma once

#include "tile_span.hpp"

#if defined(__HIPCC__)
#define GLU_RANK_FN __host__ __device__ __forceinline__
#else
#define GLU_RANK_FN inline // (a host compiler: the test program)
#endif

namespace glu_hip
{
template<uint32_t ELEM_BYTES, uint32_t PACKS>
struct SelectBatchCfg : TileCfg<ELEM_BYTES, PACKS>
{
    using C = TileCfg<ELEM_BYTES, PACKS>;
    static constexpr uint32_t LANE_BITS = C::PACKS * C::VEC; // flags of a lane
    static_assert(LANE_BITS == 8 || LANE_BITS == 16, "a lane's flag word is a byte or two");
    static constexpr uint32_t WORD_LANES = 64 / LANE_BITS;             // lanes per 64-bit word
    static constexpr uint32_t WAVE_WORDS = kTileLanes / WORD_LANES;    // 64-bit words of a wave
    static constexpr uint32_t TILE_WORDS = kTileWaves * WAVE_WORDS;    // 64-bit words of a tile: TILE / 64
    static constexpr uint32_t TILE_FLAG_BYTES = TILE_WORDS * 8;        // TILE / 8
};

// Where the batched call keeps its three arrays in one allocation, for `total` elements at any alignment: one tile more than the
// plan's (TileSpan), and one count more than tiles (the total).  Everything on a 16-byte boundary.  total == 0: nothing.
struct SelectBatchScratch
{
    size_t counts_at, below_at, flags_at, bytes;
};
inline SelectBatchScratch select_batch_scratch(uint64_t total, uint32_t elem_bytes, uint32_t packs)
{
    SelectBatchScratch s = {0, 0, 0, 0};
    if (!total) return s;
    const size_t tiles = (size_t) tile_plan(total, elem_bytes, packs).tiles + 1;
    s.counts_at = 0;
    s.below_at = ((tiles + 1) * sizeof(uint32_t) + 15) / 16 * 16;
    s.flags_at = s.below_at + tiles * kTileWaves * sizeof(uint32_t);
    s.bytes = s.flags_at + tiles * (tile_elems(elem_bytes, packs) / 8);
    return s;
}

// element v of the span's base as (tile, wave, pack, lane, element of the pack)
struct SelectBatchPos
{
    uint32_t tile, wave, pack, lane, elem;
};
template<typename C>
GLU_RANK_FN SelectBatchPos select_batch_pos(uint64_t v)
{
    SelectBatchPos p;
    p.tile = (uint32_t) (v / C::TILE);
    uint32_t r = (uint32_t) (v % C::TILE);
    p.wave = r / C::WAVE_ELEMS;
    r %= C::WAVE_ELEMS;
    p.pack = r / C::PACK_STRIDE;
    r %= C::PACK_STRIDE;
    p.lane = r / C::VEC;
    p.elem = r % C::VEC;
    return p;
}

// The flag bits of 64-bit word j (lanes j * WORD_LANES ..) of p's wave that are elements in front of position p.  Of a lane's
// flags these are: all of the packs below p's; of p's pack everything where the lane is below p's, the elements below p's in p's
// own lane, nothing in the lanes behind.  A word of lanes that are all below or all behind p's is one multiplication.
template<typename C>
GLU_RANK_FN uint64_t select_batch_word_mask(uint32_t j, const SelectBatchPos& p)
{
    constexpr uint64_t EVERY = C::LANE_BITS == 8 ? 0x0101010101010101ull : 0x0001000100010001ull; // bit 0 of every lane of a word
    const uint32_t shift = p.pack * C::VEC;                                                       // (below LANE_BITS <= 16)
    const uint64_t packs_below = ((1u << shift) - 1u) * EVERY, whole_pack = (uint64_t) (((1u << C::VEC) - 1u) << shift) * EVERY;
    const uint32_t first = j * C::WORD_LANES;
    if (first + C::WORD_LANES <= p.lane) return packs_below | whole_pack;
    if (first > p.lane) return packs_below;
    const uint32_t at = (p.lane - first) * C::LANE_BITS; // p's lane in this word (below 64)
    return packs_below | (whole_pack & ((1ull << at) - 1ull)) | ((uint64_t) (((1u << p.elem) - 1u) << shift) << at);
}

// The selected elements in front of element v of the span's base, v <= the span's hi <= tiles * TILE.  word_at(i) reads 64-bit
// word i of the flags, i < tiles * TILE_WORDS; tile_scan has tiles + 1 entries, wave_below 4 * tiles.  A position on the end of
// the last tile reads no flag at all.
template<typename C, typename WordAt>
GLU_RANK_FN uint32_t select_batch_rank(uint64_t v, uint32_t tiles, const uint32_t* tile_scan, const uint32_t* wave_below, WordAt word_at)
{
    const SelectBatchPos p = select_batch_pos<C>(v);
    if (p.tile >= tiles) return tile_scan[tiles];
    const uint32_t wave = p.tile * kTileWaves + p.wave;
    uint32_t rank = tile_scan[p.tile] + wave_below[wave];
    for (uint32_t j = 0; j < C::WAVE_WORDS; j++)
        rank += (uint32_t) __builtin_popcountll(word_at((size_t) wave * C::WAVE_WORDS + j) & select_batch_word_mask<C>(j, p));
    return rank;
}

} // namespace glu_hip
