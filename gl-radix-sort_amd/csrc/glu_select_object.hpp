// glu_select_object.hpp -- the Select object behind glu::Select (glu_select.hip owns its life and its one call).
#pragma once

#include "glu_host.hpp"

struct glu_select_s
{
    // selected elements per tile of the stencil, scanned in place by every call: 4 bytes per tile
    glu_hip::host::Scratch tile_counts;
};
