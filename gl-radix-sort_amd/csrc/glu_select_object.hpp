// glu_select_object.hpp -- the Select object behind glu::Select (glu_select.hip owns its life and its calls).
#pragma once

#include "glu_tile_host.hpp"

struct glu_select_s
{
    glu_hip::host::TileCounts tile_counts; // selected elements per tile of the stencil (the single call)
    // the batched call (select_batch_scratch): the counts per tile, the wave sums below each wave, a flag bit per element
    glu_hip::host::Scratch batch;
    void release()
    {
        tile_counts.release();
        batch.release();
    }
};
