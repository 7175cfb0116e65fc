// glu_histogram_object.hpp -- the Histogram object behind glu::Histogram (glu_histogram.hip owns its life and its calls).  The plan
// of a call is histogram_bins.hpp's hist_plan, of a batched call its hist_batch_plan.
#pragma once

#include "glu_batch_host.hpp"
#include "glu_tile_host.hpp"
#include "histogram_batch_walk.hpp"
#include "histogram_bins.hpp"

struct glu_histogram_s
{
    glu_hip::host::Scratch partial; // the rows of the LDS path: groups x bins counters
    // what the last call enqueued
    struct Last
    {
        uint32_t path = 0, groups = 0, kernels = 0;
    } last;
    // batched calls: the list image of a call with device offsets (batch_lists.hpp), the rows of the chunks of the long segments,
    // the segments per class of the last one (glu_histogram_read_batch)
    glu_hip::host::Scratch batch_lists, batch_partial;
    glu_hip::host::LastBatch last_batch;
    void release()
    {
        partial.release();
        batch_lists.release();
        batch_partial.release();
    }
};

namespace glu_hip
{
namespace host
{
// what prepare(count, bins) reserves: the most any key type and mode takes for these counts
inline size_t hist_scratch_most(uint64_t count, uint32_t bins)
{
    size_t most = 0;
    for (uint32_t key_bytes = 4; key_bytes <= 8; key_bytes += 4)
        for (int mode = HIST_EVEN; mode <= HIST_EDGES; mode++) most = std::max(most, hist_plan(count, bins, key_bytes, mode, false).scratch_bytes);
    return most;
}
} // namespace host
} // namespace glu_hip
