// histogram_kernels.hpp -- gfx950 kernels of HISTOGRAM (glu_histogram_run_even_ptr, glu_histogram_run_edges_ptr): counts of the
// samples per bin, over even bins or over sorted edges.  Not in the reference.
//
// The rules that give a sample its bin are histogram_bins.hpp (plain C++, tested on the host); the walk over the tiles, the adds and
// their skew handling (hist_walk, hist_add_bins) are histogram_walk.hpp, which top-k's counting kernels share.
//   LDS path     histogram_count_kernel: `groups` workgroups; each zeroes a table of `bins` counters in LDS (edges mode: and copies
//                the bins + 1 edges beside it), walks the tiles g, g + groups, ... adding with LDS atomics, and stores its table as
//                row g of partial[groups][bins] by contiguous lanes and plain stores.
//                histogram_sum_kernel: out[b] = (accumulate ? out[b] : 0) + the sum of column b.  Zero rows write the zeros.
//   GLOBAL path  histogram_clear_kernel (not under accumulate), then histogram_global_kernel: the same walk, adding with device-scope
//                atomics straight into out_counts.
// The kernels below are plain __global__ functions among templates: ONE translation unit (glu_histogram.hip) includes this header.
#pragma once

#include "histogram_walk.hpp"

namespace glu_hip
{
// the edges a workgroup stages: none for even bins (one element, unused)
template<typename T, typename Rule>
struct HistLdsEdges
{
    static constexpr uint32_t COUNT = 1;
};
template<typename T>
struct HistLdsEdges<T, HistEdges<T>>
{
    static constexpr uint32_t COUNT = kHistLdsBins + 1;
};

template<typename T, typename Rule, uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void histogram_count_kernel(HistArgs<T, Rule> a)
{
    __shared__ uint32_t table[kHistLdsBins];
    __shared__ T lds_edges[HistLdsEdges<T, Rule>::COUNT];
    for (uint32_t b = threadIdx.x; b < a.bins; b += THREADS) table[b] = 0u; // (bins <= kHistLdsBins: the host)
    if constexpr (std::is_same<Rule, HistEdges<T>>::value)
        for (uint32_t i = threadIdx.x; i < a.rule.n_edges; i += THREADS) lds_edges[i] = a.rule.edges[i]; // (n_edges = bins + 1)
    __syncthreads();
    // (a bin is below `bins` by its rule; checked once more in front of the table: edges that are not sorted must not reach outside)
    hist_walk<T, THREADS>(a, lds_edges, [&](uint32_t bin, uint32_t n) {
        if (bin < a.bins) atomicAdd(&table[bin], n);
    });
    __syncthreads();
    uint32_t* row = a.dst + (size_t) blockIdx.x * a.bins;
    for (uint32_t b = threadIdx.x; b < a.bins; b += THREADS) row[b] = table[b];
}

// 64 columns to the workgroup, its four waves taking the rows w, w + 4, ...
constexpr uint32_t kHistSumThreads = 256, kHistSumCols = 64;
__global__ __launch_bounds__(kHistSumThreads) void histogram_sum_kernel(const uint32_t* __restrict__ partial, uint32_t groups, uint32_t bins,
                                                                        uint32_t* __restrict__ out, uint32_t accumulate)
{
    constexpr uint32_t SLICES = kHistSumThreads / kHistSumCols;
    __shared__ uint32_t part[SLICES][kHistSumCols];
    const uint32_t col = threadIdx.x % kHistSumCols, slice = threadIdx.x / kHistSumCols;
    const uint32_t b = blockIdx.x * kHistSumCols + col;
    uint32_t sum = 0;
    if (b < bins)
    {
#pragma unroll 4
        for (uint32_t g = slice; g < groups; g += SLICES) sum += partial[(size_t) g * bins + b];
    }
    part[slice][col] = sum;
    __syncthreads();
    if (slice == 0 && b < bins)
    {
#pragma unroll
        for (uint32_t s = 1; s < SLICES; s++) sum += part[s][col];
        out[b] = (accumulate ? out[b] : 0u) + sum;
    }
}

constexpr uint32_t kHistClearThreads = 256;
__global__ __launch_bounds__(kHistClearThreads) void histogram_clear_kernel(uint32_t* __restrict__ out, uint32_t bins)
{
    const uint32_t b = blockIdx.x * kHistClearThreads + threadIdx.x;
    if (b < bins) out[b] = 0u;
}

template<typename T, typename Rule, uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void histogram_global_kernel(HistArgs<T, Rule> a)
{
    hist_walk<T, THREADS>(a, (const T*) nullptr, [&](uint32_t bin, uint32_t n) {
        if (bin < a.bins) atomicAdd(&a.dst[bin], n);
    });
}

} // namespace glu_hip
