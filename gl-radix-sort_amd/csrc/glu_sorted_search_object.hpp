// glu_sorted_search_object.hpp -- the SortedSearch object behind glu::SortedSearch (glu_sorted_search.hip owns its life and its
// calls), and the level rule of its index as the host states it.
#pragma once

#include "glu_tile_host.hpp"
#include "search_batch_walk.hpp"

struct glu_sorted_search_s
{
    glu_hip::host::Scratch index; // the levels 1 .. L of the index, each from a 128-byte boundary
    int path = GLU_SEARCH_PATH_AUTO;
    uint32_t top_entries = 0; // 0: the LDS maximum of the key width
    uint32_t batch_window = glu_hip::kSearchBatchWindowUnset; // keys staged in LDS by the batched calls; unset: the maximum of the key width
    // the haystack the index in `index` was built from
    struct Built
    {
        bool valid = false;
        const void* hay = nullptr;
        size_t hay_count = 0;
        int key_type = 0;
        uint32_t top_entries = 0;
    } built;
    // what the last call enqueued
    struct Last
    {
        uint32_t path = 0, levels = 0, kernels = 0;
    } last;
    void release() { index.release(); }
};

namespace glu_hip
{
namespace host
{
constexpr uint32_t kSearchLevelsMax = 8;     // (sorted_search_kernels.hpp: kSearchMaxLevels)
// AUTO takes the index iff needle_count * this >= hay_count.  Where forced DIRECT and forced INDEXED (build included) cross for
// random needles (profiles/sorted_search/ladder.txt): hay_count / 30 needles at 2^24 uint32 keys, / 105 at 2^28 uint32 keys, / 58
// at 2^28 uint64 keys; the sizes disagree and the larger power of two is taken.
constexpr size_t kIndexNeedleRatio = 128;

// The level rule: len_0 = hay_count, len_k = floor(hay_count / F^k); L = the smallest k with len_k <= top_entries.
struct SearchPlan
{
    uint32_t fanout, levels;
    uint32_t len[kSearchLevelsMax];
    size_t offset[kSearchLevelsMax]; // bytes from the start of the index to level k (1 .. L)
    size_t index_bytes;              // every level's room is a multiple of 128 bytes
    uint32_t entries;                // len_1 + .. + len_L
};

inline SearchPlan search_plan(size_t hay_count, uint32_t key_bytes, uint32_t top_entries)
{
    SearchPlan p = {};
    p.fanout = 128u / key_bytes;
    const uint32_t log_f = key_bytes == 4 ? 5u : 4u;
    p.len[0] = (uint32_t) hay_count;
    while (p.len[p.levels] > top_entries)
    {
        p.levels++;
        p.len[p.levels] = (uint32_t) (hay_count >> (p.levels * log_f));
        p.offset[p.levels] = p.index_bytes;
        p.index_bytes += ((size_t) p.len[p.levels] * key_bytes + 127) / 128 * 128;
        p.entries += p.len[p.levels];
    }
    return p;
}
} // namespace host
} // namespace glu_hip
