// glu_top_k_object.hpp -- the TopK object behind glu::TopK (glu_top_k.hip owns its life and its one call).
#pragma once

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
        if (sort) (void) glu_radix_sort_destroy(sort);
        sort = nullptr;
    }
};
