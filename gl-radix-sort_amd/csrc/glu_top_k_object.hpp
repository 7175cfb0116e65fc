// glu_top_k_object.hpp -- the TopK object behind glu::TopK (glu_top_k.hip owns its life and its one call, glu_top_k_batch.hip the
// batched calls).
#pragma once

#include "glu_batch_host.hpp"
#include "glu_tile_host.hpp"
#include "topk_pick.hpp"

struct glu_top_k_s
{
    glu_hip::host::Scratch state;   // TopkState, then the kTopkBins column sums of a round
    glu_hip::host::Scratch partial; // partial[groups][kTopkBins]
    glu_hip::host::Scratch cand;    // the candidates: `capacity` code words
    glu_hip::host::Scratch pairs;   // the ordering: max_k code words, then max_k indices
    glu_hip::host::TileCounts less_counts, tie_counts; // per tile: keys below the threshold word, keys equal to it
    glu_radix_sort sort = nullptr;  // orders the k pairs; prepared for max_k
    uint32_t path = glu_hip::TOPK_PATH_AUTO, capacity = 0; // the options (capacity 0: the default of the count)
    uint32_t last_kernels = 0;      // what the last run enqueued
    glu_hip::host::Scratch batch_lists; // the batched calls: the list image of a call with device offsets (batch_lists.hpp)
    glu_hip::host::Scratch batch_rows;  // ... the sorted stage: num_segments x k code words, then as many indices
    glu_hip::host::LastBatch last_batch;
    uint64_t batch_loop_min = 0;    // the option BATCH_LOOP_MIN (0: the default, topk_batch_plan.hpp)
    uint32_t last_batch_kernels = 0;
    bool ran = false;               // the state on the device is that of a run
    void* last_stream = nullptr;
    void release()
    {
        state.release();
        partial.release();
        cand.release();
        pairs.release();
        less_counts.release();
        tie_counts.release();
        batch_lists.release();
        batch_rows.release();
        if (sort) (void) glu_radix_sort_destroy(sort);
        sort = nullptr;
    }
};
