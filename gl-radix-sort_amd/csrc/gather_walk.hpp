// gather_walk.hpp -- the arithmetic of GATHER and SCATTER (gather_kernels.hpp, glu_gather.hip) in plain C++: the tile of a call,
// which position of the streaming side a (tile, wave, pack, lane, element) is, whether it lies inside the array and whether its pack
// may move whole, the row and the segment of a position of the batched forms with their clamps, and the plan.  The kernels include
// this header, and tests/test_gather_plan.py includes it with a host compiler and walks whole arrays through it: what holds there
// (every position of the array visited once and nothing outside, a whole pack only where every element moves, every begin + index
// below total, whatever the offsets and the indices hold) holds on the device.
//
// The STREAMING SIDE of a call is the array that is walked front to back: `out` of a gather, `items` of a scatter.  It moves in
// pieces of min(item_bytes, 16) bytes (a 32-byte item is two pieces, taken by two neighbouring lanes), in 16-byte packs counted from
// the 16-byte boundary at or below the array (tile_span.hpp): the array is the pieces [lo, hi) of that base.
#pragma once

#include "histogram_bins.hpp" // the exact quotient by a kernel-uniform divisor (hist_div)
#include "tile_span.hpp"

namespace glu_hip
{
constexpr uint32_t kGatherThreads = kTileThreads;
constexpr uint32_t kGatherMaxSegments = 1u << 24;    // the batched family's limit
constexpr uint64_t kGatherMaxCount = 0xFFFFFFFFull;  // count, total, num_segments * k: below 2^32
constexpr uint64_t kGatherMaxTable = 0x100000000ull; // item_count, out_count: every uint32 index can name an entry

// 16-byte packs of the streaming side per thread and tile.  PROVISIONAL, and stated here alone: 4 packs are 16 items of 4 bytes, 16
// index loads and then 16 item loads in flight per lane; the wider items keep the 64 bytes of data registers and need fewer indices.
// profiles/gather/tile_sizes.txt holds 2 and 8 beside it (a build with -DGLU_GATHER_PACKS=n, for that measurement alone).
#ifndef GLU_GATHER_PACKS
#define GLU_GATHER_PACKS 4
#endif
constexpr uint32_t gather_packs(uint32_t /*item_bytes*/) { return GLU_GATHER_PACKS; }

constexpr uint32_t gather_piece_bytes(uint32_t item_bytes) { return item_bytes < 16u ? item_bytes : 16u; }
constexpr uint32_t gather_pieces(uint32_t item_bytes) { return item_bytes / gather_piece_bytes(item_bytes); } // of an item: 1 or 2
// items per workgroup
constexpr uint32_t gather_tile(uint32_t item_bytes)
{
    return tile_elems(gather_piece_bytes(item_bytes), gather_packs(item_bytes)) / gather_pieces(item_bytes);
}

template<uint32_t ITEM_BYTES>
struct GatherCfg : TileCfg<gather_piece_bytes(ITEM_BYTES), gather_packs(ITEM_BYTES)>
{
    static constexpr uint32_t PIECE_BYTES = gather_piece_bytes(ITEM_BYTES);
    static constexpr uint32_t PIECES = gather_pieces(ITEM_BYTES);
};

// tile = items per workgroup, tiles = ceil(count / tile): the tiles of `count` items from an aligned base (one more where the
// array starts inside a pack and its end crosses into another tile), one kernel unless there is nothing to do
struct GatherPlan
{
    uint32_t tile, tiles, kernels;
};
inline GatherPlan gather_plan(uint64_t count, uint32_t item_bytes)
{
    GatherPlan p;
    p.tile = gather_tile(item_bytes);
    p.tiles = (uint32_t) ((count + p.tile - 1) / p.tile);
    p.kernels = count ? 1u : 0u;
    return p;
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------
// The first piece of pack g of `lane` of `wave` of `tile`, counted from the base: wave-major, then pack, then lane, so that a wave
// instruction covers 64 consecutive packs, 1 KiB.  The pack's pieces are first .. first + VEC - 1.
template<typename Cfg>
GLU_HIST_FN uint64_t gather_pack_first(uint32_t tile, uint32_t wave, uint32_t g, uint32_t lane)
{
    return (uint64_t) tile * Cfg::TILE + wave * Cfg::WAVE_ELEMS + g * Cfg::PACK_STRIDE + lane * Cfg::VEC;
}

// piece p of the base is a piece of the array
GLU_HIST_FN bool gather_inside(uint64_t p, uint64_t lo, uint64_t hi) { return p >= lo && p < hi; }

// every piece of the pack is one of the array: it may be loaded whole, and stored whole where none of its pieces is skipped
GLU_HIST_FN bool gather_pack_inside(uint64_t first, uint32_t vec, uint64_t lo, uint64_t hi) { return first >= lo && first + vec <= hi; }

// every piece of tile `tile` (tile_pieces of them) is one of the array: all tiles of a call but the first, where the array starts
// inside a pack, and the last
GLU_HIST_FN bool gather_tile_inside(uint32_t tile, uint32_t tile_pieces, uint64_t lo, uint64_t hi)
{
    const uint64_t first = (uint64_t) tile * tile_pieces;
    return first >= lo && first + tile_pieces <= hi;
}

// Piece p (inside) is piece `*part` of item `*item` of the array; the item is below count < 2^32.
GLU_HIST_FN void gather_item_of(uint64_t p, uint64_t lo, uint32_t pieces, uint32_t* item, uint32_t* part)
{
    const uint64_t q = p - lo;
    *item = (uint32_t) (pieces == 2u ? q >> 1 : q);
    *part = pieces == 2u ? (uint32_t) (q & 1u) : 0u;
}

// ---- the batched forms -----------------------------------------------------------------------------------------------------------
// Rows of stride k over num_segments segments: entry j = s * k + col, j < num_segments * k < 2^32.  The quotient by the
// kernel-uniform k is histogram's multiplication, exact for every j < 2^32.
struct GatherRows
{
    HistEvenInt by_k;       // magic and w_is_one for W = k; lo and span unused
    uint32_t k;             // >= 1
    uint32_t count;         // equal partitions: elements of a partition
    uint32_t total;         // elements of the items array
    uint32_t offsets_form;  // segments from device offsets
};

inline GatherRows gather_make_rows(uint32_t k, uint32_t count, uint32_t total, bool offsets_form)
{
    GatherRows r = {};
    r.by_k.lo = 0u;
    r.by_k.span = 0xFFFFFFFFu;
    r.by_k.w_is_one = k == 1u ? 1u : 0u;
    r.by_k.magic = k == 1u ? 0ull : 0xFFFFFFFFFFFFFFFFull / k + 1ull; // ceil(2^64 / k) for k >= 2
    r.k = k;
    r.count = count;
    r.total = total;
    r.offsets_form = offsets_form ? 1u : 0u;
    return r;
}

GLU_HIST_FN void gather_row(uint32_t j, const GatherRows& r, uint32_t* segment, uint32_t* col)
{
    const uint32_t s = hist_div(j, r.by_k);
    *segment = s;
    *col = j - s * r.k;
}

// Partition s of `count` elements each; s < num_partitions, so begin + len <= total < 2^32.
GLU_HIST_FN void gather_partition_segment(uint32_t s, const GatherRows& r, uint32_t* begin, uint32_t* len)
{
    *begin = s * r.count;
    *len = r.count;
}

// Segment [b, e) of device offsets, which the host cannot check: one that ends below its begin or beyond `total` is empty
// (batch_offsets_segment of batch_lists.hpp, on the two words already loaded).  Then begin + len <= total.
GLU_HIST_FN void gather_offsets_segment(uint32_t b, uint32_t e, const GatherRows& r, uint32_t* begin, uint32_t* len)
{
    if (e < b || e > r.total) e = b;
    *begin = b;
    *len = e - b;
}

// Entry `col` of a row whose segment is [begin, begin + len) and whose index word is `index`: it moves iff col < min(k, len) and
// index < len, and then from element *source = begin + index < begin + len <= total.
GLU_HIST_FN bool gather_batch_source(uint32_t begin, uint32_t len, uint32_t col, uint32_t index, const GatherRows& r, uint32_t* source)
{
    const uint32_t k_s = r.k < len ? r.k : len;
    const bool moves = col < k_s && index < len;
    *source = moves ? begin + index : 0u;
    return moves;
}

} // namespace glu_hip
