// glu_key_runs_object.hpp -- the KeyRuns object behind glu::KeyRuns (glu_key_runs.hip owns its life and its one call).
#pragma once

#include "glu_host.hpp"

struct glu_key_runs_s
{
    // heads per tile of the keys, scanned in place by every call: 4 bytes per tile
    glu_hip::host::Scratch tile_counts;
};

namespace glu_hip
{
namespace host
{
// The scan of per-tile counts that key runs and select (glu_select.hip) share, defined in glu_key_runs.hip: key_runs_scan_kernel,
// one workgroup, enqueued on `stream`.  tile_counts[0 .. tiles) becomes its exclusive scan, *total (on the device) their sum.
glu_status launch_tile_count_scan(uint32_t* tile_counts, uint32_t tiles, uint32_t* total, hipStream_t stream);
// the rounds that workgroup makes over `tiles` counts (host only)
uint32_t tile_count_scan_rounds(uint32_t tiles);
} // namespace host
} // namespace glu_hip
