// glu_scan_batch.hip -- the batched scan of libglu_hip.so (scan_batch_kernels.hpp): glu_scan_run_batch_offsets_ptr,
// glu_scan_run_batch_offsets_op_ptr, glu_scan_prepare_batch, glu_scan_plan_batch, glu_scan_read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "glu_batch_host.hpp"
#include "glu_reduce_object.hpp"
#include "glu_scan_object.hpp"
#include "scan_batch_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// the classes of a batch (the six lists of the batched reduce with this operator's limits)
BatchClasses classes_of(size_t elem_bytes)
{
    const uint32_t es = (uint32_t) elem_bytes;
    return {1, {kSbGroup4Bytes / es, kSbGroup16Bytes / es, kSbWaveBytes / es, kSbBlockBytes / es}, kSbChunkBytes / es, true};
}

// what a batch needs beside its lists: a partial per entry of the chunk list (of one element each, whatever the operator)
glu_status reserve_partials(glu_scan_s* s, const BatchListsLayout& layout, size_t elem_bytes)
{
    if (layout.capacity[BATCH_LIST_CHUNKS]) GLU_TRY(s->batch_partials.reserve((size_t) layout.capacity[BATCH_LIST_CHUNKS] * elem_bytes));
    return GLU_OK;
}

struct BatchCall
{
    glu_scan_s* scan;
    const void* data; // == out: in place
    void* out;
    size_t total, num_segments;
    const uint32_t* offsets;
    hipStream_t stream;
};

// The counts cleared, binning, one kernel for the three short lists, one for the medium list, three for the long segments (chunk
// sums, the scan of every segment's partials, the chunks with their carry-in): seven enqueued operations at most, and which of
// them are enqueued depends on `total` and `num_segments` alone (a class whose list cannot hold a segment is skipped).
template<int OP, bool INCLUSIVE, bool IN_PLACE, typename S, int N>
glu_status run_offsets(const BatchCall& c)
{
    using T = Elem<S, N>;
    static_assert(!IN_PLACE || (OP == OP_SUM && !INCLUSIVE), "the in-place kernels are the exclusive `+` scan");
    glu_scan_s* s = c.scan;
    BatchListsArgs a = {};
    uint32_t *counts, *lists, bin_grid;
    GLU_TRY(begin_batch_offsets(s->batch_lists, classes_of(sizeof(T)), c.total, c.num_segments, c.stream, a.layout, counts, lists, bin_grid));
    GLU_TRY(reserve_partials(s, a.layout, sizeof(T)));
    a.offsets = c.offsets;
    a.total = (uint32_t) c.total;
    a.nsegs = (uint32_t) c.num_segments;
    a.counts = counts;
    a.lists = lists;
    const T* data = (const T*) c.data;
    T* out = (T*) c.out;
    T* partials = (T*) s->batch_partials.ptr;
    // (no `out`, elements of no words: the reduce's binning kernel writes no identities and only lists)
    hipLaunchKernelGGL(reduce_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, c.stream, a, counts, lists, (uint32_t*) nullptr, 0u,
                       ReduceBatchIdentity{});
    HIP_TRY(hipGetLastError());
    s->last_batch.on_device = true;
    // IN_PLACE: the kernels of the exclusive `+` scan in place; otherwise those with an operator, a kind and a store pointer
    const auto wave = [&](dim3 grid) {
        if constexpr (IN_PLACE) hipLaunchKernelGGL((scan_batch_wave_kernel<S, N>), grid, dim3(kSbThreads), 0, c.stream, out, a);
        else hipLaunchKernelGGL((scan_ops_wave_kernel<OP, INCLUSIVE, S, N>), grid, dim3(kSbThreads), 0, c.stream, data, out, a);
    };
    const auto block = [&](dim3 grid, int mode) {
        if constexpr (IN_PLACE) hipLaunchKernelGGL((scan_batch_block_kernel<S, N>), grid, dim3(kSbThreads), 0, c.stream, out, partials, a, mode);
        else hipLaunchKernelGGL((scan_ops_block_kernel<OP, INCLUSIVE, S, N>), grid, dim3(kSbThreads), 0, c.stream, data, out, partials, a, mode);
    };
    wave(dim3(3u * short_lists_blocks(a.layout, kSbWaves)));
    HIP_TRY(hipGetLastError());
    if (a.layout.capacity[BATCH_LIST_BLOCK])
    {
        block(dim3(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_BLOCK], cus() * 8u)), (int) SB_MODE_SEGMENTS);
        HIP_TRY(hipGetLastError());
    }
    if (a.layout.capacity[BATCH_LIST_LONG])
    {
        const dim3 chunk_grid(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_CHUNKS], cus() * 8u));
        hipLaunchKernelGGL((reduce_batch_chunk_kernel<OP, S, N>), chunk_grid, dim3(kRbThreads), 0, c.stream, data, partials, a, (uint64_t) 0);
        HIP_TRY(hipGetLastError());
        block(dim3(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_LONG], cus() * 8u)), (int) SB_MODE_PARTIALS);
        HIP_TRY(hipGetLastError());
        block(chunk_grid, (int) SB_MODE_CHUNKS);
        HIP_TRY(hipGetLastError());
    }
    return GLU_OK;
}

// the exclusive `+` scan in place: the kernels glu_scan_run_batch_offsets_ptr has always run
struct BatchRunner
{
    BatchCall call;
    template<typename S, int N>
    glu_status operator()()
    {
        return run_offsets<OP_SUM, false, true, S, N>(call);
    }
};

// an operator, a kind and a store pointer
template<int OP>
struct OpRunner
{
    BatchCall call;
    bool inclusive;
    template<typename S, int N>
    glu_status operator()()
    {
        return inclusive ? run_offsets<OP, true, false, S, N>(call) : run_offsets<OP, false, false, S, N>(call);
    }
};

glu_status run_op(const BatchCall& c, glu_reduce_operator op, bool inclusive)
{
    const glu_data_type type = c.scan->type;
    switch (op)
    {
    case GLU_REDUCE_SUM: return dispatch_type(type, OpRunner<OP_SUM>{c, inclusive});
    case GLU_REDUCE_MUL: return dispatch_type(type, OpRunner<OP_MUL>{c, inclusive});
    case GLU_REDUCE_MIN: return dispatch_type(type, OpRunner<OP_MIN>{c, inclusive});
    case GLU_REDUCE_MAX: return dispatch_type(type, OpRunner<OP_MAX>{c, inclusive});
    default: return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid reduce operator: %d", (int) op);
    }
}

// the two offset words of the one-segment form (offsets == NULL)
glu_status reserve_whole_offsets(glu_scan_s* s) { return s->batch_whole.reserve(2 * sizeof(uint32_t)); }

} // namespace

extern "C" {

glu_status glu_scan_plan_batch(size_t count, uint32_t elem_bytes, uint32_t* path, uint32_t* workgroups)
{
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16 && elem_bytes != 32)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "elem_bytes must be 4, 8, 16 or 32 (got %u)", elem_bytes);
    uint32_t p, w;
    scan_batch_plan(count, elem_bytes, p, w);
    store(path, p);
    store(workgroups, w);
    return GLU_OK;
}

glu_status glu_scan_prepare_batch(glu_scan scan, size_t total, size_t num_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(scan, "scan"));
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    const size_t elem_bytes = data_type_size(scan->type);
    BatchListsLayout layout;
    GLU_TRY(reserve_batch_lists(scan->batch_lists, classes_of(elem_bytes), total, num_segments, layout));
    GLU_TRY(reserve_whole_offsets(scan));
    return reserve_partials(scan, layout, elem_bytes);
}

glu_status glu_scan_run_batch_offsets_ptr(glu_scan scan, void* data, size_t total, const uint32_t* offsets, size_t num_segments,
                                          void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(scan, "scan"));
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    if (num_segments == 0)
    {
        scan->last_batch.reset();
        return GLU_OK;
    }
    if (total && !data) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid data buffer");
    GLU_TRY(check_batch_offsets(offsets, num_segments));
    GLU_TRY(check_aligned(data, std::min<size_t>(16, data_type_size(scan->type)), "data", "its element size"));
    if (total == 0) // every segment is empty
    {
        scan->last_batch.reset();
        return GLU_OK;
    }
    BatchRunner r{{scan, data, data, total, num_segments, offsets, pick_stream(stream)}};
    return dispatch_type(scan->type, r);
}

glu_status glu_scan_run_batch_offsets_op_ptr(glu_scan scan, const void* data, void* out, size_t total, const uint32_t* offsets,
                                             size_t num_segments, glu_reduce_operator op, glu_scan_kind kind, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(scan, "scan"));
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    if ((int) op < (int) GLU_REDUCE_SUM || (int) op >= (int) GLU_REDUCE_COUNT_) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid reduce operator: %d", (int) op);
    if (kind != GLU_SCAN_EXCLUSIVE && kind != GLU_SCAN_INCLUSIVE) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid scan kind: %d", (int) kind);
    if (!offsets && num_segments > 1) return fail(GLU_ERROR_INVALID_ARGUMENT, "NULL offsets mean one segment (got %zu)", num_segments);
    if (num_segments == 0)
    {
        scan->last_batch.reset();
        return GLU_OK;
    }
    if (total && !data) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid data buffer");
    GLU_TRY(check_aligned(offsets, sizeof(uint32_t), "the offsets array", "its element size"));
    const size_t elem_bytes = data_type_size(scan->type);
    GLU_TRY(check_aligned(data, std::min<size_t>(16, elem_bytes), "data", "its element size"));
    GLU_TRY(check_aligned(out, std::min<size_t>(16, elem_bytes), "out", "its element size"));
    if (!out) out = const_cast<void*>(data);
    if (out != data) GLU_TRY(check_disjoint({{out, total * elem_bytes, "out"}}, {{data, total * elem_bytes, "data"}}));
    if (total == 0) // every segment is empty
    {
        scan->last_batch.reset();
        return GLU_OK;
    }
    const hipStream_t st = pick_stream(stream);
    if (!offsets)
    {
        GLU_TRY(reserve_whole_offsets(scan));
        uint32_t* whole = (uint32_t*) scan->batch_whole.ptr;
        hipLaunchKernelGGL(scan_batch_whole_offsets_kernel, dim3(1), dim3(64), 0, st, whole, (uint32_t) total);
        HIP_TRY(hipGetLastError());
        offsets = whole;
    }
    const BatchCall c{scan, data, out, total, num_segments, offsets, st};
    if (op == GLU_REDUCE_SUM && kind == GLU_SCAN_EXCLUSIVE && out == data) return dispatch_type(scan->type, BatchRunner{c});
    return run_op(c, op, kind == GLU_SCAN_INCLUSIVE);
}

glu_status glu_scan_read_batch(glu_scan scan, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(scan, "scan"));
    return scan->last_batch.read(scan->batch_lists, 3, wave_segments, block_segments, long_segments); // (the three short lists)
}

} // extern "C"
