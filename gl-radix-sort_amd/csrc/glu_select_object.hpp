// glu_select_object.hpp -- the Select object behind glu::Select (glu_select.hip owns its life and its one call).
#pragma once

#include "glu_tile_host.hpp"

struct glu_select_s
{
    glu_hip::host::TileCounts tile_counts; // selected elements per tile of the stencil
    void release() { tile_counts.release(); }
};
