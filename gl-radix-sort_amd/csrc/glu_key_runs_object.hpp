// glu_key_runs_object.hpp -- the KeyRuns object behind glu::KeyRuns (glu_key_runs.hip owns its life and its one call).
#pragma once

#include "glu_tile_host.hpp"

struct glu_key_runs_s
{
    glu_hip::host::TileCounts tile_counts; // heads per tile of the keys
    void release() { tile_counts.release(); }
};
