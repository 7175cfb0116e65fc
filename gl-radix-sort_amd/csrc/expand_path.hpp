// expand_path.hpp -- the arithmetic of EXPAND (expand_kernels.hpp, glu_expand.hip) in plain C++: the tile of a call, the cut of the
// merged sequence at a tile boundary, the ranges of a tile with their clamps, the indices into the tile's two LDS arrays and the
// bound on the segment index a gather uses.  Both expand kernels include this header, and tests/test_expand_path.py includes it with
// a host compiler and expands whole arrays through it: what holds there (every offset index below num_segments + 1, every output
// below total, every LDS index inside its array, every gathered segment below num_segments, whatever the offsets hold) holds on the
// device.
//
// Expand is a load-balancing search: merge path (merge_path.hpp) between the offsets, side A, na = num_segments + 1 values, and
// the counting sequence 0 .. total - 1, side B, nb = total positions.  A comes first on ties, which is the rule "offsets[r] <= j":
// in the merged sequence the offsets in front of position j are exactly the r with offsets[r] <= j, c(j) of them.
#pragma once

#include "merge_path.hpp"

namespace glu_hip
{
constexpr uint32_t kExpandThreads = 256;
// Merged items (offsets + positions) per thread and tile.  Odd: a thread scans ITEMS consecutive words of LDS, and neighbouring
// lanes start ITEMS words apart.  profiles/expand/tile_sizes.txt holds the neighbours.
constexpr uint32_t kExpandItems = 11;
constexpr uint32_t kExpandTile = kExpandThreads * kExpandItems;
constexpr uint32_t kExpandMaxSegments = 1u << 24;    // the batched family's limit
constexpr uint64_t kExpandMaxMerged = 0xFFFFFFFFull; // (num_segments + 1) + total <= 2^32 - 1: a merged index is a word

// the tile boundary t = 0 .. tiles of a merged sequence of `merged` items
GLU_MERGE_FN uint32_t expand_diag(uint32_t t, uint32_t merged)
{
    const uint64_t d64 = (uint64_t) t * kExpandTile;
    return d64 < merged ? (uint32_t) d64 : merged;
}

// How many offsets lie among the first d items of the merged sequence (d <= na + nb): merge_diag_split with the positions as side
// B.  offset_at(i, any) is called with i < na where `any`.  max(0, d - nb) <= the result <= min(d, na) whatever the offsets hold.
template<typename OffsetAt>
GLU_MERGE_FN uint32_t expand_split(uint32_t d, uint32_t na, uint32_t nb, OffsetAt offset_at)
{
    return merge_diag_split(d, na, nb, merge_steps(na < nb ? na : nb), offset_at, [](uint32_t j, bool) { return j; });
}

// Tile t holds the offsets [a0, a1) and the positions [b0, b1): 0 <= a0 <= a1 <= na, 0 <= b0 <= b1 <= nb and
// (a1 - a0) + (b1 - b0) <= kExpandTile, by merge_tile_ranges' clamp, whatever the offsets hold.
GLU_MERGE_FN MergeRanges expand_tile_ranges(uint32_t split0, uint32_t split1, uint32_t t, uint32_t merged)
{
    return merge_tile_ranges(split0, split1, expand_diag(t, merged), expand_diag(t + 1u, merged));
}

// The tile's slice of the offsets in LDS, kExpandTile + 1 words: slot k = 0 .. a1 - a0 holds offsets[a0 + k - 1], so slot 0 is the
// offset in front of the tile (none where a0 == 0: the slot is never used then, expand_segment).  `*has`: there is such an offset;
// the index returned is below a1 <= na.
GLU_MERGE_FN uint32_t expand_slice_source(uint32_t a0, uint32_t k, bool* has)
{
    *has = a0 + k != 0u;
    return *has ? a0 + k - 1u : 0u;
}

// Slot k = 1 .. na_t of the slice holds the value v, the next slot `next` (read only where k < na_t).  The last offset of a run of
// equal ones marks the position it equals, if that is one of the tile's nb_t positions: word v - b0 of the marks, nb_t <=
// kExpandTile words, takes k.  With sorted offsets a run never straddles a tile (the offsets equal to v all lie in front of position
// v), so every word has one writer.
GLU_MERGE_FN bool expand_marks(uint32_t k, uint32_t na_t, uint32_t v, uint32_t next, uint32_t b0, uint32_t nb_t, uint32_t* mark_index)
{
    const bool last = k == na_t || next != v;
    const uint32_t i = v - b0; // (wraps where v < b0: then not below nb_t)
    *mark_index = i < nb_t ? i : 0u;
    return last && i < nb_t;
}

// Position b0 + i of the tile: `scanned` is the inclusive maximum of marks[0 .. i], every mark a slot 0 .. na_t, so
// c = a0 + scanned <= a1 <= na offsets lie at or in front of the position.  It is covered iff 1 <= c <= num_segments; its segment
// c - 1 is then below num_segments by this test and not by what the offsets hold, and slot `scanned` of the slice holds
// offsets[c - 1] (c >= 1: slot 0 is filled where a0 > 0).
GLU_MERGE_FN bool expand_segment(uint32_t a0, uint32_t scanned, uint32_t num_segments, uint32_t* segment)
{
    const uint32_t c = a0 + scanned;
    const bool covered = c >= 1u && c <= num_segments;
    *segment = covered ? c - 1u : 0u;
    return covered;
}

} // namespace glu_hip
