// tile_count_scan_kernel.hpp -- the middle kernel of key runs and select (tile_compact_kernels.hpp).  A plain __global__, so one
// translation unit includes this header: glu_key_runs.hip, which defines host::launch_tile_count_scan (glu_tile_host.hpp) for both.
#pragma once

#include "scan_batch_kernels.hpp"

namespace glu_hip
{
// One workgroup.  tile_counts[0 .. tiles) becomes its exclusive scan by scan_batch_range -- the tile loop that scan_batch_block_kernel
// runs over a long segment's partials, 4096 counts per round (kTileScanRound) with a running carry -- and *total their sum, or
// `most` if that is less (set operations on keys that are not sorted; everyone else passes 2^32 - 1).
__global__ __launch_bounds__(kSbThreads) void key_runs_scan_kernel(uint32_t* __restrict__ tile_counts, uint32_t tiles,
                                                                   uint32_t* __restrict__ total, uint32_t most)
{
    using T = Elem<uint32_t, 1>;
    __shared__ T wsum[2][kSbWaves];
    __shared__ uint32_t last;
    if (threadIdx.x == 0) last = tiles ? tile_counts[tiles - 1] : 0u;
    __syncthreads();
    uint32_t phase = 0;
    scan_batch_range<OP_SUM, false, uint32_t, 1, false, true>(nullptr, reinterpret_cast<T*>(tile_counts), tiles, zero_elem<uint32_t, 1>(), threadIdx.x,
                                                              wsum, phase);
    __syncthreads(); // (the last count's scan was stored by another thread of this workgroup)
    if (threadIdx.x == 0)
    {
        const uint32_t sum = tiles ? tile_counts[tiles - 1] + last : 0u;
        *total = sum < most ? sum : most;
    }
}

} // namespace glu_hip
