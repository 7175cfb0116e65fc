// glu_key_runs_object.hpp -- the KeyRuns object behind glu::KeyRuns (glu_key_runs.hip owns its life and its one call).
#pragma once

#include "glu_host.hpp"

struct glu_key_runs_s
{
    // heads per tile of the keys, scanned in place by every call: 4 bytes per tile
    glu_hip::host::Scratch tile_counts;
};
