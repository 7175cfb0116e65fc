// topk_batch_plan.hpp -- the plan of BATCHED TOP-K (topk_batch_kernels.hpp, glu_top_k_batch.hip) in plain C++: the length classes
// and their limits, the digit windows of a select at any digit width (the wave class takes narrower digits than topk_pick.hpp's 11
// bits), the rule of the loop over single calls, the kernels a call enqueues and the scratch it takes.  The kernels and the host
// include this header, and tests/test_top_k_batch_plan.py includes it with a host compiler and runs whole selects through it.
// THE CLASS LIMITS, THE WAVE CLASS'S DIGIT WIDTH, THE CANDIDATE ROOM AND THE LOOP THRESHOLD ARE PROVISIONAL: no ladder row sits at a
// class limit, and the loop threshold is the crossover measured at 64 rows only (profiles/top_k_batch/README.md).  This header is
// their single statement; tests read them through glu_top_k_plan_batch and never hard-code them.
#pragma once

#include "batch_lists.hpp"
#include "topk_pick.hpp"

namespace glu_hip
{
constexpr uint32_t kTopkBatchWaveKpt = 8;                           // keys a lane of the wave class holds, consecutive ones
constexpr uint32_t kTopkBatchWaveTile = 64u * kTopkBatchWaveKpt;    // 512: the longest segment of the wave class
constexpr uint32_t kTopkBatchWaveWaves = 4;                         // waves (= segments in flight) per workgroup of the wave class
constexpr uint32_t kTopkBatchWaveDigitBits = 8;                     // digit width of the wave class: a row of 256 counters per wave
// code words a workgroup tile holds in LDS, in bytes (tile 0 .. 2), and the threads of its workgroup
constexpr uint32_t topk_batch_tile_bytes(int tile) { return tile == 0 ? 8u << 10 : tile == 1 ? 32u << 10 : 128u << 10; }
constexpr uint32_t topk_batch_tile_threads(int tile) { return tile == 0 ? 256u : 1024u; }
constexpr uint32_t kTopkBatchLongThreads = 1024;
constexpr uint32_t kTopkBatchCandBytes = 32u << 10;                 // the long class's candidate buffer in LDS, in bytes
constexpr uint64_t kTopkBatchLoopMinDefault = (uint64_t) 1 << 22;   // partitions this long go through the single call, one by one
constexpr int kTopkBatchLists = BATCH_LIST_LONG + 1;                // wave, three tiles, long: one-word entries, no chunks

// ---- digit windows of a select with digits of `width` bits, taken from the top (width == kTopkDigitBits: topk_pick.hpp's own)
GLU_TOPK_FN uint32_t topk_rounds_w(uint32_t key_bytes, uint32_t width) { return (key_bytes * 8u + width - 1u) / width; }
GLU_TOPK_FN uint32_t topk_shift_w(uint32_t key_bytes, uint32_t width, uint32_t r)
{
    const uint32_t key_bits = key_bytes * 8u, top = width * (r + 1u);
    return top < key_bits ? key_bits - top : 0u;
}
GLU_TOPK_FN uint32_t topk_bits_w(uint32_t key_bytes, uint32_t width, uint32_t r)
{
    const uint32_t left = key_bytes * 8u - width * r;
    return left < width ? left : width;
}
// topk_advance at that width: round r ended at digit d, which holds count_d words behind `before` others
GLU_TOPK_FN void topk_advance_w(TopkState& s, uint32_t key_bytes, uint32_t width, uint32_t r, uint32_t d, uint32_t before, uint32_t count_d)
{
    const uint32_t shift = topk_shift_w(key_bytes, width, r), bits = topk_bits_w(key_bytes, width, r);
    s.prefix |= (uint64_t) d << shift;
    s.mask |= (uint64_t) ((1u << bits) - 1u) << shift;
    s.less += before;
    s.need -= before;
    s.bucket = count_d;
}

// ---- the classes.  List c of batch_lists.hpp: 0 the wave class, 1 .. 3 the three workgroup tiles, 4 (BATCH_LIST_LONG) the rest.
GLU_TOPK_FN uint32_t topk_batch_limit(int c, uint32_t key_bytes) { return c == 0 ? kTopkBatchWaveTile : topk_batch_tile_bytes(c - 1) / key_bytes; }
GLU_TOPK_FN int topk_batch_class(uint64_t len, uint32_t key_bytes)
{
    for (int c = 0; c < BATCH_LIST_LONG; c++)
        if (len <= topk_batch_limit(c, key_bytes)) return c;
    return BATCH_LIST_LONG;
}
GLU_TOPK_FN uint32_t topk_batch_cand_room(uint32_t key_bytes) { return kTopkBatchCandBytes / key_bytes; }
// a segment of one key has an answer: every non-empty segment is listed
inline BatchClasses topk_batch_classes(uint32_t key_bytes)
{
    return {1, {topk_batch_limit(0, key_bytes), topk_batch_limit(1, key_bytes), topk_batch_limit(2, key_bytes), topk_batch_limit(3, key_bytes)}, 0, false};
}

enum
{
    TOPK_BATCH_NONE = 0, // nothing is enqueued
    TOPK_BATCH_WAVE,     // equal partitions: the one class kernel the host picked
    TOPK_BATCH_BLOCK,
    TOPK_BATCH_LONG,
    TOPK_BATCH_LOOP,     // equal partitions of at least loop_min keys: glu_top_k_run_ptr, partition after partition
    TOPK_BATCH_BINNED    // device offsets: the binning kernel, then one kernel per class that can hold a segment
};

struct TopkBatchPlan
{
    uint32_t path, tile, kernels;
    int list;             // equal partitions on a class kernel: its list (0 .. BATCH_LIST_LONG), else -1
    size_t scratch_bytes; // the list image (device offsets), the rows of pairs (arrays and sorted); LOOP: the single call's
};

// offsets_form: `count` is the batch's total.  loop_min: 0 = the default.  rows_sorted_singly: k is beyond the batched sort's
// single-block limit, the ordering is one ordinary sort per row (the caller asks glu_radix_sort_plan_batch).  single: the plan of
// one glu_top_k_run_ptr(count, k) under the object's options (LOOP).  Kernels:
//   equal partitions      the class kernel                                                   1
//   LOOP                  single.kernels per partition
//   device offsets        the binning kernel, one kernel per list that can hold a segment    1 + (1 .. 5)
//   arrays and sorted     the object's batched sort (counted as one; one per row where rows_sorted_singly), the decode kernel
inline TopkBatchPlan topk_batch_plan(bool offsets_form, uint64_t count, uint64_t num_segments, uint64_t k, uint32_t key_bytes, bool arrays,
                                     bool sorted, uint64_t loop_min, bool rows_sorted_singly, const TopkPlan& single)
{
    TopkBatchPlan p = {TOPK_BATCH_NONE, 0, 0, -1, 0};
    if (!count || !num_segments || !k) return p;
    if (!loop_min) loop_min = kTopkBatchLoopMinDefault;
    const uint32_t ordering = arrays && sorted ? (uint32_t) (rows_sorted_singly ? num_segments : 1u) + 1u : 0u;
    const size_t rows = arrays && sorted ? (size_t) (num_segments * k) * (key_bytes + sizeof(uint32_t)) : 0;
    if (offsets_form)
    {
        size_t words;
        const BatchListsLayout l = batch_lists_layout(topk_batch_classes(key_bytes), count, num_segments, words);
        p.path = TOPK_BATCH_BINNED;
        p.kernels = 1u + ordering;
        for (int c = 0; c <= BATCH_LIST_LONG; c++) p.kernels += l.capacity[c] ? 1u : 0u;
        p.scratch_bytes = (64 + words) * sizeof(uint32_t) + rows; // (64: the line of counts, glu_batch_host.hpp)
        return p;
    }
    if (count >= loop_min)
    {
        p.path = TOPK_BATCH_LOOP;
        p.kernels = (uint32_t) num_segments * single.kernels;
        p.scratch_bytes = single.scratch_bytes;
        return p;
    }
    p.list = topk_batch_class(count, key_bytes);
    p.path = p.list == 0 ? TOPK_BATCH_WAVE : p.list == BATCH_LIST_LONG ? TOPK_BATCH_LONG : TOPK_BATCH_BLOCK;
    p.tile = p.list == BATCH_LIST_LONG ? 0u : topk_batch_limit(p.list, key_bytes);
    p.kernels = 1u + ordering;
    p.scratch_bytes = rows;
    return p;
}

} // namespace glu_hip
