// glu_scan_object.hpp -- the BlellochScan object, shared by the translation units behind glu::BlellochScan: glu_scan_reduce.hip owns
// its life and the single scan, glu_scan_batch.hip its batched calls.
#pragma once

#include "glu_batch_host.hpp"
#include "scan_reduce_kernels.hpp"

struct glu_scan_s
{
    glu_data_type type;
    glu_hip::host::Scratch sums;
    // chained (single-pass) scan state for 4-byte element types: one 64-bit word per chunk + a ticket counter
    glu_hip::host::Scratch chain;
    glu_hip::host::Scratch ticket;
    uint32_t epoch = 0;
    bool chained = true; // GLU_HIP_SCAN_CHAINED=0 falls back to reduce-then-scan
    size_t chain_min_chunks = glu_hip::kChainMinChunks; // GLU_HIP_SCAN_CHAINED=2: chained from 2 chunks up (tests)
    // the batched scan: the list counts and the segment lists of a call; the per-chunk partials of long segments
    glu_hip::host::Scratch batch_lists;
    glu_hip::host::Scratch batch_partials;
    glu_hip::host::Scratch batch_whole; // the two offset words of the one-segment form, written on the device
    glu_hip::host::LastBatch last_batch; // segments per class of the last batched call (glu_scan_read_batch)
    void release()
    {
        for (glu_hip::host::Scratch* s : {&sums, &chain, &ticket, &batch_lists, &batch_partials, &batch_whole}) s->release();
    }
};
