// histogram_batch_kernels.hpp -- gfx950 kernels of the BATCHED HISTOGRAM (glu_histogram_run_batch_*_ptr): every segment of an array
// counted into a row of its own, out_counts[s * bins + b] = the samples of segment s in bin b.  Not in the reference.
//
// A sample gets its bin by the rules of the single call (histogram_bins.hpp), the adds and their skew handling are
// histogram_walk.hpp's (hist_add_bins, HistPending), the segment lists, their layout and the clamps are batch_lists.hpp's, and what
// decides which memory is touched is histogram_batch_walk.hpp (plain C++, walked on the host by tests/test_histogram_batch_walk.py).
// Three classes by the length of a segment (hist_batch_plan draws the lines):
//   wave   histogram_batch_wave_kernel   a wave per segment, four to a workgroup, each with a table of `bins` <= 2048 counters of its
//                                        own in LDS; the row is written by contiguous lanes.
//   block  histogram_batch_block_kernel  a workgroup per segment, the table (and the staged edges) of histogram_count_kernel.
//   long   the same kernel over the entries (segment, chunk) of the chunk list: the table goes to partial[slot][bins] in the object's
//          scratch; histogram_batch_sum_kernel then adds every long segment's rows: out = (accumulate ? out : 0) + their sum.
// histogram_batch_bin_kernel in front (device offsets only) appends every segment to the list of its class and zeroes the rows of the
// empty ones.  Every table lives in LDS, where skew costs nothing; NO GLOBAL ATOMICS ON COUNTS: the only global atomics are the list
// appends of the shared layer.  Counts are integers: the same input gives the same bits whatever the arrival order.
// The kernels below are plain __global__ functions among templates: ONE translation unit (glu_histogram.hip) includes this header.
#pragma once

#include "histogram_batch_walk.hpp"
#include "histogram_kernels.hpp"

namespace glu_hip
{
// A batched call as its kernels see it (l: reduce_batch_kernels.hpp's BatchListsArgs, the segments and the lists)
template<typename T, typename Rule>
struct HistBatchArgs
{
    const T* samples; // sample 0 of the batch
    Rule rule;
    uint32_t bins;
    uint32_t accumulate;
    uint32_t* out;     // out_counts[nsegs][bins]
    uint32_t* partial; // partial[slot][bins], the rows of the chunks of the long segments
    BatchListsArgs l;
};

// (the clamp of a segment is the shared layer's: batch_clamp_segment behind hist_batch_segment)
__device__ __forceinline__ void hist_batch_segment_of(const BatchListsArgs& l, uint32_t seg, uint64_t& begin, uint64_t& len)
{
    hist_batch_segment(l.offsets != nullptr, [&](uint32_t i) { return l.offsets[i]; }, l.count, l.total, seg, begin, len);
}

// ---------------------------------------------------------------------------------------------------------
// Binning (device offsets), one lane per segment: the segment appended to the list of its class, a long one with an entry per chunk.
// Where the call does not accumulate, the rows of the empty segments are zeroed by the WHOLE WAVE, row after row of the ballot over
// its empty lanes, bins / 64 stores a lane: a row can be 32 KiB, which one lane must not write by itself.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void histogram_batch_bin_kernel(BatchListsArgs l, uint32_t* __restrict__ counts, uint32_t* __restrict__ lists,
                                                                  uint32_t* __restrict__ out, uint32_t bins, uint32_t accumulate)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * 256u; base < l.nsegs; base += gridDim.x * 256u) // (workgroup-uniform; nsegs <= 2^24)
    {
        const uint32_t seg = base + threadIdx.x;
        int cls = -1;
        uint32_t nchunks = 0;
        bool empty = false;
        if (seg < l.nsegs)
        {
            uint64_t begin, len;
            hist_batch_segment_of(l, seg, begin, len);
            cls = hist_batch_class(len, l.layout.limit[BATCH_LIST_SHORT4], l.layout.limit[BATCH_LIST_BLOCK]);
            if (cls == BATCH_LIST_LONG) nchunks = hist_batch_chunks(len, l.layout.chunk);
            empty = len == 0;
        }
        batch_append<BATCH_LIST_LONG>(cls, seg, lane, l.layout, counts, lists);
        batch_append_long(cls == BATCH_LIST_LONG, seg, nchunks, lane, l.layout, counts, lists);
        uint64_t m = accumulate ? 0ull : __ballot(empty);
        while (m) // wave-uniform
        {
            const uint32_t src = (uint32_t) __ffsll((unsigned long long) m) - 1u;
            m &= m - 1;
            uint32_t* row = out + hist_batch_row(seg - lane + src, bins); // (lane `src` holds a segment below nsegs: it is empty)
            for (uint32_t b = lane; b < bins; b += 64u) row[b] = 0u;
        }
    }
}

// out[0 .. n) = 0: equal partitions of no samples
__global__ __launch_bounds__(256) void histogram_batch_clear_kernel(uint32_t* __restrict__ out, uint64_t n)
{
    for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t) gridDim.x * 256u) out[i] = 0u;
}

// the edges a workgroup of the wave class stages: bins <= kHistBatchWaveBins there
template<typename T, typename Rule>
struct HistBatchWaveEdges
{
    static constexpr uint32_t COUNT = 1;
};
template<typename T>
struct HistBatchWaveEdges<T, HistEdges<T>>
{
    static constexpr uint32_t COUNT = kHistBatchWaveBins + 1;
};

// the bins of the calling thread's packs p0 + g * STRIDE (g < kHistPacks) of a span, added: packs behind the span's last are masked
// as the samples in front of and behind the segment are (tile_load_pack reads no element outside [lo, hi))
template<typename T, uint32_t STRIDE, typename Rule, typename Add>
__device__ __forceinline__ void hist_batch_add_packs(const TileSpan<T>& span, uint32_t p0, const Rule& rule, const T* lds_edges, HistPending& pending,
                                                     Add add)
{
    constexpr uint32_t VEC = 16 / sizeof(T), N = kHistPacks * VEC;
    T x[N];
    uint32_t inside = 0;
#pragma unroll
    for (uint32_t g = 0; g < kHistPacks; g++)
        tile_load_pack<VEC>(span, ((uint64_t) p0 + g * STRIDE) * VEC, [&](uint32_t k, T v, bool in) {
            x[g * VEC + k] = v;
            inside |= (in ? 1u : 0u) << (g * VEC + k);
        });
    uint32_t bin[N];
#pragma unroll
    for (uint32_t e = 0; e < N; e++) bin[e] = (inside >> e) & 1u ? hist_bin_of(rule, x[e], lds_edges) : kHistNoBin;
    hist_add_bins<N>(bin, pending, add);
}

// ---------------------------------------------------------------------------------------------------------
// Wave class: wave w of workgroup g takes the entries (g * 4 + w), + 4 * gridDim.x, ... of the wave list (or of the partitions).
// ---------------------------------------------------------------------------------------------------------
template<typename T, typename Rule>
__global__ __launch_bounds__(256) void histogram_batch_wave_kernel(HistBatchArgs<T, Rule> a)
{
    static_assert(kHistBatchWaves * 64u == 256u, "four waves to the workgroup");
    __shared__ uint32_t tables[kHistBatchWaves][kHistBatchWaveBins];
    __shared__ T lds_edges[HistBatchWaveEdges<T, Rule>::COUNT];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if constexpr (std::is_same<Rule, HistEdges<T>>::value)
        for (uint32_t i = threadIdx.x; i < a.rule.n_edges; i += 256u) lds_edges[i] = a.rule.edges[i]; // (n_edges <= 2049: the host)
    __syncthreads(); // the only workgroup barrier: the waves take different numbers of segments, so there is NONE inside the loop
    uint32_t* table = tables[wave];
    const uint32_t n = a.l.lists ? batch_list_length(a.l.counts, a.l.layout, BATCH_LIST_SHORT4) : a.l.nsegs;
    const uint32_t* list = a.l.lists ? a.l.lists + a.l.layout.start[BATCH_LIST_SHORT4] : nullptr;
    const auto add = [&](uint32_t bin, uint32_t count) {
        if (bin < a.bins) atomicAdd(&table[bin], count); // (checked once more in front of the table, as in histogram_count_kernel)
    };
    for (uint64_t li = (uint64_t) blockIdx.x * kHistBatchWaves + wave; li < n; li += (uint64_t) gridDim.x * kHistBatchWaves) // (wave-uniform)
    {
        const uint32_t seg = (uint32_t) __builtin_amdgcn_readfirstlane((int) (list ? list[li] : (uint32_t) li));
        uint64_t begin, len;
        hist_batch_segment_of(a.l, seg, begin, len);
        for (uint32_t b = lane; b < a.bins; b += 64u) table[b] = 0u;
        const TileSpan<T> span = hist_batch_span(a.samples, begin, len);
        HistPending pending; // starts empty for every segment
        for (uint32_t p0 = 0; p0 < span.tiles; p0 += 64u * kHistPacks) // (wave-uniform)
            hist_batch_add_packs<T, 64u>(span, p0 + lane, a.rule, lds_edges, pending, add);
        pending.flush(add); // flushed at the end of EVERY segment, before the row is read back: no add crosses to the next segment
        // adds before read-back: the LDS operations of one wave execute in issue order, and the wavefront fence with the wave
        // barrier keeps the compiler from moving the reads of the table above the adds (or the next zeroing above the reads)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t* row = a.out + hist_batch_row(seg, a.bins);
        if (a.accumulate)
            for (uint32_t b = lane; b < a.bins; b += 64u) row[b] += table[b];
        else
            for (uint32_t b = lane; b < a.bins; b += 64u) row[b] = table[b];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------------------
// Block class (chunks == 0): a workgroup per entry of the block list (or per partition); its table is the row of the segment.
// Long class (chunks == 1): a workgroup per entry (segment, chunk) of the chunk list (or per (partition, chunk) pair, `items` of
// them); its table is row `slot` of the partials, a plain store whatever the call's accumulate says.
// The table, the edge staging and the threads per mode are histogram_count_kernel's.
// ---------------------------------------------------------------------------------------------------------
template<typename T, typename Rule, uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void histogram_batch_block_kernel(HistBatchArgs<T, Rule> a, uint32_t chunks, uint64_t items)
{
    __shared__ uint32_t table[kHistLdsBins];
    __shared__ T lds_edges[HistLdsEdges<T, Rule>::COUNT];
    if constexpr (std::is_same<Rule, HistEdges<T>>::value)
        for (uint32_t i = threadIdx.x; i < a.rule.n_edges; i += THREADS) lds_edges[i] = a.rule.edges[i]; // (n_edges = bins + 1)
    const int c = chunks ? BATCH_LIST_CHUNKS : BATCH_LIST_BLOCK;
    const uint64_t n = a.l.lists ? (uint64_t) batch_list_length(a.l.counts, a.l.layout, c) : items;
    const auto add = [&](uint32_t bin, uint32_t count) {
        if (bin < a.bins) atomicAdd(&table[bin], count);
    };
    for (uint64_t li = blockIdx.x; li < n; li += gridDim.x) // (workgroup-uniform)
    {
        uint32_t seg, chunk = 0;
        if (!chunks) seg = a.l.lists ? a.l.lists[a.l.layout.start[BATCH_LIST_BLOCK] + li] : (uint32_t) li;
        else if (a.l.lists)
        {
            const uint2 entry = reinterpret_cast<const uint2*>(a.l.lists + a.l.layout.start[BATCH_LIST_CHUNKS])[li];
            seg = entry.x;
            chunk = entry.y;
        }
        else
        {
            seg = (uint32_t) (li / a.l.chunks_per);
            chunk = (uint32_t) (li % a.l.chunks_per);
        }
        uint64_t begin, len;
        hist_batch_segment_of(a.l, seg, begin, len);
        if (chunks)
        {
            uint64_t at;
            uint32_t part;
            hist_batch_chunk_range(len, chunk, a.l.layout.chunk, at, part);
            begin += at;
            len = part;
        }
        for (uint32_t b = threadIdx.x; b < a.bins; b += THREADS) table[b] = 0u; // (bins <= kHistLdsBins: the host)
        __syncthreads();
        const TileSpan<T> span = hist_batch_span(a.samples, begin, len);
        HistPending pending;
        for (uint32_t p0 = 0; p0 < span.tiles; p0 += THREADS * kHistPacks) // (workgroup-uniform)
            hist_batch_add_packs<T, THREADS>(span, p0 + threadIdx.x, a.rule, lds_edges, pending, add);
        pending.flush(add);
        __syncthreads();
        // (li is below the list's capacity, so a slot's row lies inside the reserved partials; a segment's row inside out_counts)
        uint32_t* row = chunks ? a.partial + hist_batch_row(li, a.bins) : a.out + hist_batch_row(seg, a.bins);
        if (!chunks && a.accumulate)
            for (uint32_t b = threadIdx.x; b < a.bins; b += THREADS) row[b] += table[b];
        else
            for (uint32_t b = threadIdx.x; b < a.bins; b += THREADS) row[b] = table[b];
        __syncthreads(); // the table is zeroed again in the next round
    }
}

// ---------------------------------------------------------------------------------------------------------
// Long class, second step: blockIdx.y, + gridDim.y, ... walk the long list (or the partitions); 64 columns to the workgroup, its
// four waves taking the rows w, w + 4, ... of the segment's run of partials, as in histogram_sum_kernel.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHistSumThreads) void histogram_batch_sum_kernel(BatchListsArgs l, const uint32_t* __restrict__ partial,
                                                                              uint32_t* __restrict__ out, uint32_t bins, uint32_t accumulate)
{
    constexpr uint32_t SLICES = kHistSumThreads / kHistSumCols;
    __shared__ uint32_t part[SLICES][kHistSumCols];
    const uint32_t col = threadIdx.x % kHistSumCols, slice = threadIdx.x / kHistSumCols;
    const uint32_t b = blockIdx.x * kHistSumCols + col;
    const uint32_t n = l.lists ? batch_list_length(l.counts, l.layout, BATCH_LIST_LONG) : l.nsegs;
    for (uint32_t li = blockIdx.y; li < n; li += gridDim.y) // (workgroup-uniform)
    {
        uint32_t seg = li, rows = l.chunks_per;
        uint64_t slot = (uint64_t) li * l.chunks_per;
        if (l.lists)
        {
            const uint2 entry = reinterpret_cast<const uint2*>(l.lists + l.layout.start[BATCH_LIST_LONG])[li];
            seg = entry.x;
            slot = entry.y;
            uint64_t begin, len;
            hist_batch_segment_of(l, seg, begin, len);
            rows = hist_batch_chunks(len, l.layout.chunk); // (a listed segment's whole run lies inside the chunk list)
        }
        uint32_t sum = 0;
        if (b < bins)
        {
#pragma unroll 4
            for (uint32_t r = slice; r < rows; r += SLICES) sum += partial[hist_batch_row(slot + r, bins) + b];
        }
        part[slice][col] = sum;
        __syncthreads();
        if (slice == 0 && b < bins)
        {
#pragma unroll
            for (uint32_t s = 1; s < SLICES; s++) sum += part[s][col];
            uint32_t* row = out + hist_batch_row(seg, bins);
            row[b] = (accumulate ? row[b] : 0u) + sum;
        }
        __syncthreads(); // `part` is written again in the next round
    }
}

} // namespace glu_hip
