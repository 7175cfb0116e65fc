// glu_expand_object.hpp -- the Expand object behind glu::Expand (glu_expand.hip owns its life and its calls), and the plan of a call
// as the host states it.
#pragma once

#include "expand_path.hpp"
#include "glu_tile_host.hpp"

struct glu_expand_s
{
    glu_hip::host::Scratch split; // the split table of a call: (tiles + 1) words
    // what the last call enqueued
    struct Last
    {
        uint32_t tiles = 0, kernels = 0;
    } last;
    void release() { split.release(); }
};

namespace glu_hip
{
namespace host
{
// tile = merged items (offsets + positions) per workgroup, tiles = ceil((num_segments + 1 + total) / tile), two kernels and the
// split table, unless there is no position or no segment: then nothing
struct ExpandPlan
{
    uint32_t tile, tiles, kernels;
    size_t scratch_bytes;
};

inline ExpandPlan expand_plan(uint64_t total, uint64_t num_segments)
{
    ExpandPlan p;
    const uint64_t merged = total && num_segments ? num_segments + 1 + total : 0;
    p.tile = kExpandTile;
    p.tiles = (uint32_t) ((merged + p.tile - 1) / p.tile);
    p.kernels = merged ? 2u : 0u;
    p.scratch_bytes = merged ? ((size_t) p.tiles + 1) * sizeof(uint32_t) : 0;
    return p;
}
} // namespace host
} // namespace glu_hip
