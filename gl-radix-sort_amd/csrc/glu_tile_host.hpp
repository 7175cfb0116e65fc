// glu_tile_host.hpp -- what glu_key_runs.hip and glu_select.hip share on the host side: the tile counts an operator object owns,
// the grid of the streaming kernels and the launch of the count scan.  (The limit of a call and the overlap test: glu_args.hpp.)
#pragma once

#include <algorithm>

#include "glu_batch_host.hpp"
#include "tile_span.hpp"

namespace glu_hip
{
namespace host
{
// Flags per tile of an array, scanned in place by every call: 4 bytes per tile.  What glu_key_runs_s and glu_select_s are.
struct TileCounts : Scratch
{
    // for `count` elements at any alignment: one tile more than the plan's (TileSpan)
    glu_status reserve(size_t count, uint32_t elem_bytes, uint32_t packs)
    {
        return count ? Scratch::reserve(((size_t) tile_plan(count, elem_bytes, packs).tiles + 1) * sizeof(uint32_t)) : GLU_OK;
    }
};

// workgroups of a streaming kernel that walks `tiles` tiles in a loop
inline uint32_t tile_grid(uint32_t tiles) { return std::max(1u, std::min(tiles, cus() * 8u)); }

// The count scan, defined in glu_key_runs.hip (the one unit that holds key_runs_scan_kernel): one workgroup, enqueued on `stream`.
// tile_counts[0 .. tiles) becomes its exclusive scan, *total (on the device) their sum, held to `most`.
glu_status launch_tile_count_scan(uint32_t* tile_counts, uint32_t tiles, uint32_t* total, hipStream_t stream, uint32_t most = 0xFFFFFFFFu);
} // namespace host
} // namespace glu_hip
