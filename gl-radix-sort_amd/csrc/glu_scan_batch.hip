// glu_scan_batch.hip -- the batched scan of libglu_hip.so (scan_batch_kernels.hpp): glu_scan_run_batch_offsets_ptr,
// glu_scan_prepare_batch, glu_scan_plan_batch, glu_scan_read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "glu_host.hpp"
#include "glu_reduce_object.hpp"
#include "glu_scan_object.hpp"
#include "scan_batch_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
constexpr size_t kBatchMaxSegments = (size_t) 1 << 24;
constexpr uint32_t kBatchCountWords = 64; // the list counts in front of the lists, on a line of their own

// The lists of a batch (the batched reduce's six lists with this operator's limits).  A segment list can hold as many segments as
// fit `total` at its class's shortest length; the long list as many segments longer than the medium class; the chunk list a chunk
// per whole chunk of `total` and one more per long segment (its last, partial one).
ReduceBatchLayout lists_layout(size_t total, size_t num_segments, size_t elem_bytes, size_t& words)
{
    ReduceBatchLayout l;
    l.limit[RB_LIST_SHORT4] = kSbGroup4Bytes / (uint32_t) elem_bytes;
    l.limit[RB_LIST_SHORT16] = kSbGroup16Bytes / (uint32_t) elem_bytes;
    l.limit[RB_LIST_SHORT64] = kSbWaveBytes / (uint32_t) elem_bytes;
    l.limit[RB_LIST_BLOCK] = kSbBlockBytes / (uint32_t) elem_bytes;
    l.chunk = kSbChunkBytes / (uint32_t) elem_bytes;
    size_t at = 0;
    for (int c = 0; c <= RB_LIST_BLOCK; c++)
    {
        const size_t shortest = c == 0 ? 1 : (size_t) l.limit[c - 1] + 1;
        l.start[c] = (uint32_t) at;
        l.capacity[c] = (uint32_t) std::min<size_t>(num_segments, total / shortest);
        at += l.capacity[c];
    }
    at = (at + 1) & ~(size_t) 1; // the entries of the last two lists are 8 bytes
    l.start[RB_LIST_LONG] = (uint32_t) at;
    l.capacity[RB_LIST_LONG] = (uint32_t) std::min<size_t>(num_segments, total / ((size_t) l.limit[RB_LIST_BLOCK] + 1));
    at += 2 * (size_t) l.capacity[RB_LIST_LONG];
    l.start[RB_LIST_CHUNKS] = (uint32_t) at;
    l.capacity[RB_LIST_CHUNKS] = l.capacity[RB_LIST_LONG] ? (uint32_t) (total / l.chunk + l.capacity[RB_LIST_LONG]) : 0u;
    at += 2 * (size_t) l.capacity[RB_LIST_CHUNKS];
    words = kBatchCountWords + at;
    return l;
}

inline uint32_t cus() { return (uint32_t) g_dev.num_cus; }

glu_status reserve_batch(glu_scan_s* s, size_t total, size_t num_segments, size_t elem_bytes, ReduceBatchLayout& layout)
{
    size_t words;
    layout = lists_layout(total, num_segments, elem_bytes, words);
    GLU_TRY(s->batch_lists.reserve(words * sizeof(uint32_t)));
    if (layout.capacity[RB_LIST_CHUNKS]) GLU_TRY(s->batch_partials.reserve((size_t) layout.capacity[RB_LIST_CHUNKS] * elem_bytes));
    return GLU_OK;
}

struct BatchCall
{
    glu_scan_s* scan;
    void* data;
    size_t total, num_segments;
    const uint32_t* offsets;
    hipStream_t stream;
};

// The counts cleared, binning, one kernel for the three short lists, one for the medium list, three for the long segments (chunk
// sums, the scan of every segment's partials, the chunks with their carry-in): seven enqueued operations at most, and which of
// them are enqueued depends on `total` and `num_segments` alone (a class whose list cannot hold a segment is skipped).
template<typename S, int N>
glu_status run_offsets(const BatchCall& c)
{
    using T = Elem<S, N>;
    glu_scan_s* s = c.scan;
    ReduceBatchArgs a = {};
    GLU_TRY(reserve_batch(s, c.total, c.num_segments, sizeof(T), a.layout));
    uint32_t* const image = (uint32_t*) s->batch_lists.ptr;
    a.offsets = c.offsets;
    a.total = (uint32_t) c.total;
    a.nsegs = (uint32_t) c.num_segments;
    a.counts = image;
    a.lists = image + kBatchCountWords;
    T* data = (T*) c.data;
    T* partials = (T*) s->batch_partials.ptr;
    HIP_TRY(hipMemsetAsync(image, 0, kBatchCountWords * sizeof(uint32_t), c.stream));
    const uint32_t bin_grid = std::min<uint32_t>((a.nsegs + 255u) / 256u, cus() * 4u);
    // (no `out`, elements of no words: the reduce's binning kernel writes no identities and only lists)
    hipLaunchKernelGGL(reduce_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, c.stream, a, image, image + kBatchCountWords, (uint32_t*) nullptr,
                       0u, ReduceBatchIdentity{});
    HIP_TRY(hipGetLastError());
    s->last_batch_on_device = true;
    // a third of the grid per short list: a workgroup's four waves hold 64 / 16 / 4 segments of the three lists at a time
    uint32_t short_blocks = 1;
    for (int l = RB_LIST_SHORT4; l <= RB_LIST_SHORT64; l++)
    {
        const uint32_t per_block = kSbWaves * (l == RB_LIST_SHORT4 ? 16u : l == RB_LIST_SHORT16 ? 4u : 1u);
        short_blocks = std::max<uint32_t>(short_blocks, (uint32_t) (((uint64_t) a.layout.capacity[l] + per_block - 1) / per_block));
    }
    short_blocks = std::min<uint32_t>(short_blocks, cus() * 8u);
    hipLaunchKernelGGL((scan_batch_wave_kernel<S, N>), dim3(3u * short_blocks), dim3(kSbThreads), 0, c.stream, data, a);
    HIP_TRY(hipGetLastError());
    if (a.layout.capacity[RB_LIST_BLOCK])
    {
        hipLaunchKernelGGL((scan_batch_block_kernel<S, N>), dim3(std::min<uint32_t>(a.layout.capacity[RB_LIST_BLOCK], cus() * 8u)),
                           dim3(kSbThreads), 0, c.stream, data, partials, a, (int) SB_MODE_SEGMENTS);
        HIP_TRY(hipGetLastError());
    }
    if (a.layout.capacity[RB_LIST_LONG])
    {
        const dim3 chunk_grid(std::min<uint32_t>(a.layout.capacity[RB_LIST_CHUNKS], cus() * 8u));
        hipLaunchKernelGGL((reduce_batch_chunk_kernel<OP_SUM, S, N>), chunk_grid, dim3(kRbThreads), 0, c.stream, (const T*) data, partials, a,
                           (uint64_t) 0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((scan_batch_block_kernel<S, N>), dim3(std::min<uint32_t>(a.layout.capacity[RB_LIST_LONG], cus() * 8u)),
                           dim3(kSbThreads), 0, c.stream, data, partials, a, (int) SB_MODE_PARTIALS);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((scan_batch_block_kernel<S, N>), chunk_grid, dim3(kSbThreads), 0, c.stream, data, partials, a, (int) SB_MODE_CHUNKS);
        HIP_TRY(hipGetLastError());
    }
    return GLU_OK;
}

struct BatchRunner
{
    BatchCall call;
    template<typename S, int N>
    glu_status operator()()
    {
        return run_offsets<S, N>(call);
    }
};

glu_status check_sizes(size_t total, size_t num_segments)
{
    if (total >= ((size_t) 1 << 32)) return fail(GLU_ERROR_INVALID_ARGUMENT, "a batch with offsets must hold fewer than 2^32 elements (got %zu)", total);
    if (num_segments > kBatchMaxSegments) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments %zu exceeds 2^24", num_segments);
    return GLU_OK;
}
} // namespace

extern "C" {

glu_status glu_scan_plan_batch(size_t count, uint32_t elem_bytes, uint32_t* path, uint32_t* workgroups)
{
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16 && elem_bytes != 32)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "elem_bytes must be 4, 8, 16 or 32 (got %u)", elem_bytes);
    uint32_t p, w;
    scan_batch_plan(count, elem_bytes, p, w);
    if (path) *path = p;
    if (workgroups) *workgroups = w;
    return GLU_OK;
}

glu_status glu_scan_prepare_batch(glu_scan scan, size_t total, size_t num_segments)
{
    GLU_TRY(enter());
    if (!scan) return fail(GLU_ERROR_INVALID_ARGUMENT, "scan is NULL");
    GLU_TRY(check_sizes(total, num_segments));
    ReduceBatchLayout layout;
    return reserve_batch(scan, total, num_segments, data_type_size(scan->type), layout);
}

glu_status glu_scan_run_batch_offsets_ptr(glu_scan scan, void* data, size_t total, const uint32_t* offsets, size_t num_segments,
                                          void* stream)
{
    GLU_TRY(enter());
    if (!scan) return fail(GLU_ERROR_INVALID_ARGUMENT, "scan is NULL");
    GLU_TRY(check_sizes(total, num_segments));
    if (num_segments == 0)
    {
        scan->last_batch_on_device = false;
        return GLU_OK;
    }
    if (total && !data) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid data buffer");
    if (!offsets) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid offsets array");
    if ((uintptr_t) offsets % sizeof(uint32_t)) return fail(GLU_ERROR_INVALID_ARGUMENT, "the offsets array is not aligned to its element size");
    if ((uintptr_t) data % std::min<size_t>(16, data_type_size(scan->type)))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "data is not aligned to its element size");
    if (total == 0) // every segment is empty
    {
        scan->last_batch_on_device = false;
        return GLU_OK;
    }
    BatchRunner r{{scan, data, total, num_segments, offsets, pick_stream(stream)}};
    return dispatch_type(scan->type, r);
}

glu_status glu_scan_read_batch(glu_scan scan, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments)
{
    GLU_TRY(enter());
    if (!scan) return fail(GLU_ERROR_INVALID_ARGUMENT, "scan is NULL");
    uint32_t by_class[3] = {0, 0, 0};
    if (scan->last_batch_on_device)
    {
        uint32_t counts[kRbCounts];
        HIP_TRY(hipMemcpy(counts, scan->batch_lists.ptr, sizeof(counts), hipMemcpyDeviceToHost));
        by_class[0] = counts[RB_LIST_SHORT4] + counts[RB_LIST_SHORT16] + counts[RB_LIST_SHORT64];
        by_class[1] = counts[RB_LIST_BLOCK];
        by_class[2] = counts[kRbCountLong];
    }
    if (wave_segments) *wave_segments = by_class[0];
    if (block_segments) *block_segments = by_class[1];
    if (long_segments) *long_segments = by_class[2];
    return GLU_OK;
}

} // extern "C"
