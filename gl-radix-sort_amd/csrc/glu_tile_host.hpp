// glu_tile_host.hpp -- what glu_key_runs.hip and glu_select.hip share on the host side: the limit of a call, the overlap test of
// two arrays, the tile counts an operator object owns, the grid of the streaming kernels and the launch of the count scan.
#pragma once

#include <algorithm>

#include "glu_batch_host.hpp"
#include "tile_span.hpp"

namespace glu_hip
{
namespace host
{
// `what`: the operator's own sentence, e.g. "select takes a count below 2^32"
inline glu_status check_tile_count(size_t count, const char* what)
{
    return count < ((size_t) 1 << 32) ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "%s (got %zu)", what, count);
}

inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

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
// tile_counts[0 .. tiles) becomes its exclusive scan, *total (on the device) their sum.
glu_status launch_tile_count_scan(uint32_t* tile_counts, uint32_t tiles, uint32_t* total, hipStream_t stream);
} // namespace host
} // namespace glu_hip
