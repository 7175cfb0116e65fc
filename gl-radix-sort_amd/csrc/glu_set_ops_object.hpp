// glu_set_ops_object.hpp -- the SetOps object behind glu::SetOps (glu_merge.hip owns its life and its calls), the limit of a call and
// the plan of a call as the host states it.
#pragma once

#include "glu_merge_object.hpp"
#include "set_ops_path.hpp"

struct glu_set_ops_s
{
    // the scratch of a call: (tiles + 1) boundaries of three words, then the tiles' counts; of a batched call (tiles + 1) boundaries
    // of four words, the tiles' counts, then one word per thread and tile
    glu_hip::host::Scratch scratch;
    // what the last call enqueued
    struct Last
    {
        uint32_t tiles = 0, kernels = 0;
    } last;
    void release() { scratch.release(); }
};

namespace glu_hip
{
namespace host
{
constexpr uint64_t kSetOpsMaxTotal = kMergeMaxTotal; // a_count + b_count <= 2^32 - 1: merge's tiles, an output index is a word

// tile and tiles are merge's.  Kernels: bounds, count, scan, write; without the write where nothing can be written; the scan alone
// (it writes *num_out = 0) where there is nothing to look at.
struct SetOpsPlan
{
    uint32_t tile, tiles, kernels;
    size_t scratch_bytes;
};

inline SetOpsPlan set_ops_plan(uint64_t total, uint32_t key_bytes, bool with_arrays)
{
    SetOpsPlan p;
    p.tile = merge_tile(key_bytes, true);
    p.tiles = (uint32_t) ((total + p.tile - 1) / p.tile);
    p.kernels = total ? (with_arrays ? 4u : 3u) : 1u;
    p.scratch_bytes = total ? ((size_t) p.tiles + 1) * sizeof(SetBounds) + (size_t) p.tiles * sizeof(uint32_t) : 0;
    return p;
}

// The batched call (set_ops_batch_kernels.hpp): merge's tile over the host-known total.  Kernels: bounds, count, scan, then the
// offsets kernel where out_offsets is given and the write kernel where something can be written; with no keys the scan (it writes
// *num_out = 0) and the offsets kernel; with no segments the scan alone.  Scratch: (tiles + 1) boundaries of four words, the tiles'
// counts, and -- unless the call only counts and has no out_offsets, so that nobody reads them -- one word per thread and tile.
inline SetOpsPlan set_ops_batch_plan(uint64_t total, uint64_t num_segments, uint32_t key_bytes, bool with_arrays, bool with_offsets)
{
    SetOpsPlan p;
    p.tile = merge_tile(key_bytes, true);
    p.tiles = (uint32_t) ((total + p.tile - 1) / p.tile);
    const uint32_t offsets = with_offsets ? 1u : 0u;
    p.kernels = !num_segments ? 1u : (!p.tiles ? 1u + offsets : 3u + offsets + (with_arrays ? 1u : 0u));
    p.scratch_bytes = !p.tiles ? 0
                               : ((size_t) p.tiles + 1) * 4 * sizeof(uint32_t) + (size_t) p.tiles * sizeof(uint32_t) +
                                     ((with_arrays || with_offsets) ? (size_t) p.tiles * kMergeThreads * sizeof(uint32_t) : 0);
    return p;
}
} // namespace host
} // namespace glu_hip
