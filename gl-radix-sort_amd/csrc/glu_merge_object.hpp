// glu_merge_object.hpp -- the Merge object behind glu::Merge (glu_merge.hip owns its life and its calls), and the plan of a call as
// the host states it.
#pragma once

#include "glu_tile_host.hpp"
#include "merge_path.hpp"

struct glu_merge_s
{
    glu_hip::host::Scratch split; // the split table of a call: (tiles + 1) words; of a batched call (tiles + 1) boundaries of two
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
constexpr uint64_t kMergeMaxTotal = 0xFFFFFFFFull; // a_count + b_count <= 2^32 - 1: an output index is a word

// tile = outputs per workgroup, tiles = ceil(total / tile), two kernels unless there is nothing to do, the split table
struct MergePlan
{
    uint32_t tile, tiles, kernels;
    size_t scratch_bytes;
};

inline MergePlan merge_plan(uint64_t total, uint32_t key_bytes, bool with_vals)
{
    MergePlan p;
    p.tile = merge_tile(key_bytes, with_vals);
    p.tiles = (uint32_t) ((total + p.tile - 1) / p.tile);
    p.kernels = total ? 2u : 0u;
    p.scratch_bytes = total ? ((size_t) p.tiles + 1) * sizeof(uint32_t) : 0;
    return p;
}

// The batched merge (merge_batch_kernels.hpp): the single call's tile over the host-known total; the partition kernel runs whenever
// there are segments (it also writes out_offsets), the tile kernel where there are tiles; a boundary is two words (split, segment).
inline MergePlan merge_batch_plan(uint64_t total, uint64_t num_segments, uint32_t key_bytes, bool with_vals)
{
    MergePlan p;
    p.tile = merge_tile(key_bytes, with_vals);
    p.tiles = (uint32_t) ((total + p.tile - 1) / p.tile);
    p.kernels = num_segments ? (p.tiles ? 2u : 1u) : 0u;
    p.scratch_bytes = ((size_t) p.tiles + 1) * 2 * sizeof(uint32_t);
    return p;
}
} // namespace host
} // namespace glu_hip
