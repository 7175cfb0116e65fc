// glu_set_ops_object.hpp -- the SetOps object behind glu::SetOps (glu_merge.hip owns its life and its calls), the limit of a call and
// the plan of a call as the host states it.
#pragma once

#include "glu_merge_object.hpp"
#include "set_ops_path.hpp"

struct glu_set_ops_s
{
    // the scratch of a call: (tiles + 1) boundaries of three words, then the tiles' counts
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
} // namespace host
} // namespace glu_hip
