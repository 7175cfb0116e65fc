// glu_reduce_batch.hip -- the batched reduce of libglu_hip.so (reduce_batch_kernels.hpp): glu_reduce_run_batch_ptr,
// glu_reduce_run_batch_offsets_ptr, glu_reduce_prepare_batch, glu_reduce_plan_batch, glu_reduce_read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <type_traits>

#include "glu_batch_host.hpp"
#include "glu_reduce_object.hpp"
#include "reduce_batch_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// the classes of a batch with device offsets
BatchClasses classes_of(size_t elem_bytes)
{
    const uint32_t es = (uint32_t) elem_bytes;
    return {1, {kRbGroup4Elems, kRbGroup16Elems, kRbWaveBytes / es, kRbBlockBytes / es}, kRbChunkBytes / es, true};
}

template<int OP, typename S, int N>
ReduceBatchIdentity identity_of()
{
    S v;
    if (OP == OP_SUM) v = (S) 0;
    else if (OP == OP_MUL) v = (S) 1;
    else if (std::is_floating_point<S>::value) v = OP == OP_MIN ? std::numeric_limits<S>::infinity() : -std::numeric_limits<S>::infinity();
    else v = OP == OP_MIN ? std::numeric_limits<S>::max() : std::numeric_limits<S>::lowest();
    ReduceBatchIdentity id = {};
    static_assert(sizeof(S) * N <= sizeof(id.w), "an element is at most eight words");
    for (int i = 0; i < N; i++) memcpy((char*) id.w + i * sizeof(S), &v, sizeof(S));
    return id;
}

// which short list (= group size) equal partitions of `count` elements take
inline int short_sub(size_t count) { return count <= kRbGroup4Elems ? BATCH_LIST_SHORT4 : count <= kRbGroup16Elems ? BATCH_LIST_SHORT16 : BATCH_LIST_SHORT64; }

struct BatchCall
{
    glu_reduce_s* red;
    const void* data;
    void* out;
    size_t count, num_segments, total; // equal partitions: count x num_segments; device offsets: total, num_segments
    const uint32_t* offsets;
    hipStream_t stream;
};

template<int OP, typename S, int N>
glu_status run_equal(const BatchCall& c)
{
    using T = Elem<S, N>;
    glu_reduce_s* r = c.red;
    uint32_t path, workgroups;
    reduce_batch_plan(c.count, sizeof(T), path, workgroups);
    r->last_batch.reset();
    if (path) r->last_batch.by_class[path - 1] = (uint32_t) c.num_segments;
    BatchListsArgs a = {};
    a.count = c.count;
    a.nsegs = (uint32_t) c.num_segments;
    a.layout.chunk = kRbChunkBytes / (uint32_t) sizeof(T);
    const T* data = (const T*) c.data;
    T* out = (T*) c.out;
    if (path == 0)
    {
        const uint32_t grid = std::min<uint32_t>((a.nsegs + 255u) / 256u, cus() * 4u);
        hipLaunchKernelGGL(reduce_batch_fill_kernel, dim3(grid), dim3(256), 0, c.stream, (uint32_t*) c.out, a.nsegs, (uint32_t) (sizeof(T) / 4),
                           identity_of<OP, S, N>());
    }
    else if (path == 1)
    {
        a.sub = short_sub(c.count);
        const uint32_t per_block = kRbWaves * (a.sub == BATCH_LIST_SHORT4 ? 16u : a.sub == BATCH_LIST_SHORT16 ? 4u : 1u);
        const uint32_t grid = (uint32_t) std::min<uint64_t>(((uint64_t) a.nsegs + per_block - 1) / per_block, cus() * 8u);
        hipLaunchKernelGGL((reduce_batch_wave_kernel<OP, S, N>), dim3(grid), dim3(kRbThreads), 0, c.stream, data, out, a);
    }
    else if (path == 2)
    {
        const uint32_t grid = std::min<uint32_t>(a.nsegs, cus() * 8u);
        hipLaunchKernelGGL((reduce_batch_block_kernel<OP, S, N>), dim3(grid), dim3(kRbThreads), 0, c.stream, data, out, a, 0);
    }
    else
    {
        const uint64_t items = (uint64_t) workgroups * c.num_segments;
        if (workgroups == 0xFFFFFFFFu || items > 0xFFFFFFFFull) return fail(GLU_ERROR_INVALID_ARGUMENT, "the batch has too many chunks");
        GLU_TRY(r->batch_partials.reserve(items * sizeof(T)));
        a.chunks_per = workgroups;
        T* partials = (T*) r->batch_partials.ptr;
        hipLaunchKernelGGL((reduce_batch_chunk_kernel<OP, S, N>), dim3((uint32_t) std::min<uint64_t>(items, cus() * 8u)), dim3(kRbThreads), 0,
                           c.stream, data, partials, a, items);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((reduce_batch_block_kernel<OP, S, N>), dim3(std::min<uint32_t>(a.nsegs, cus() * 8u)), dim3(kRbThreads), 0, c.stream,
                           (const T*) partials, out, a, 1);
    }
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// what a batch with device offsets needs beside its lists: the partials of the long segments' chunks
glu_status reserve_partials(glu_reduce_s* r, size_t total, size_t num_segments, const BatchListsLayout& layout, size_t elem_bytes)
{
    // (equal partitions of the long class: at most total / chunk + num_segments chunks, and they are longer than a chunk)
    const size_t slots = total / layout.chunk + std::min<size_t>(num_segments, total / layout.chunk);
    if (slots) GLU_TRY(r->batch_partials.reserve(slots * elem_bytes));
    return GLU_OK;
}

// device offsets: the counts cleared, binning, one kernel for the three short lists, one for the medium list, two for the long
// segments: six launches whatever the segments look like
template<int OP, typename S, int N>
glu_status run_offsets(const BatchCall& c)
{
    using T = Elem<S, N>;
    glu_reduce_s* r = c.red;
    BatchListsArgs a = {};
    uint32_t *counts, *lists, bin_grid;
    GLU_TRY(begin_batch_offsets(r->batch_lists, classes_of(sizeof(T)), c.total, c.num_segments, c.stream, a.layout, counts, lists, bin_grid));
    GLU_TRY(reserve_partials(r, c.total, c.num_segments, a.layout, sizeof(T)));
    a.offsets = c.offsets;
    a.total = (uint32_t) c.total;
    a.nsegs = (uint32_t) c.num_segments;
    a.counts = counts;
    a.lists = lists;
    const T* data = (const T*) c.data;
    T* out = (T*) c.out;
    T* partials = (T*) r->batch_partials.ptr;
    hipLaunchKernelGGL(reduce_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, c.stream, a, counts, lists, (uint32_t*) c.out,
                       (uint32_t) (sizeof(T) / 4), identity_of<OP, S, N>());
    HIP_TRY(hipGetLastError());
    r->last_batch.on_device = true;
    if (c.total == 0) return GLU_OK; // every segment is empty
    hipLaunchKernelGGL((reduce_batch_wave_kernel<OP, S, N>), dim3(3u * short_lists_blocks(a.layout, kRbWaves)), dim3(kRbThreads), 0, c.stream,
                       data, out, a);
    HIP_TRY(hipGetLastError());
    if (a.layout.capacity[BATCH_LIST_BLOCK])
    {
        hipLaunchKernelGGL((reduce_batch_block_kernel<OP, S, N>), dim3(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_BLOCK], cus() * 8u)),
                           dim3(kRbThreads), 0, c.stream, data, out, a, 0);
        HIP_TRY(hipGetLastError());
    }
    if (a.layout.capacity[BATCH_LIST_LONG])
    {
        hipLaunchKernelGGL((reduce_batch_chunk_kernel<OP, S, N>), dim3(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_CHUNKS], cus() * 8u)),
                           dim3(kRbThreads), 0, c.stream, data, partials, a, (uint64_t) 0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((reduce_batch_block_kernel<OP, S, N>), dim3(std::min<uint32_t>(a.layout.capacity[BATCH_LIST_LONG], cus() * 8u)),
                           dim3(kRbThreads), 0, c.stream, (const T*) partials, out, a, 1);
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
        const bool offsets = call.offsets != nullptr;
        switch (call.red->op)
        {
        case GLU_REDUCE_SUM: return offsets ? run_offsets<OP_SUM, S, N>(call) : run_equal<OP_SUM, S, N>(call);
        case GLU_REDUCE_MUL: return offsets ? run_offsets<OP_MUL, S, N>(call) : run_equal<OP_MUL, S, N>(call);
        case GLU_REDUCE_MIN: return offsets ? run_offsets<OP_MIN, S, N>(call) : run_equal<OP_MIN, S, N>(call);
        case GLU_REDUCE_MAX: return offsets ? run_offsets<OP_MAX, S, N>(call) : run_equal<OP_MAX, S, N>(call);
        default: return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid reduction operator: %d", (int) call.red->op);
        }
    }
};

// what the host can check of the two arrays: `elements` of data are read, `results` of out written
glu_status check_arrays(const glu_reduce_s* r, const void* data, const void* out, size_t elements, size_t results)
{
    const size_t es = data_type_size(r->type);
    const size_t align = std::min<size_t>(16, es);
    if (elements && !data) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid data buffer");
    if (results && !out) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid output buffer");
    GLU_TRY(check_aligned(data, align, "data", "its element size"));
    GLU_TRY(check_aligned(out, align, "out", "its element size"));
    if (elements > ((size_t) -1) / es) return fail(GLU_ERROR_INVALID_ARGUMENT, "the batch is larger than the address space");
    return check_disjoint({{out, results * es, "out"}}, {{data, elements * es, "data"}});
}
} // namespace

extern "C" {

glu_status glu_reduce_plan_batch(size_t count, uint32_t elem_bytes, uint32_t* path, uint32_t* workgroups)
{
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16 && elem_bytes != 32)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "elem_bytes must be 4, 8, 16 or 32 (got %u)", elem_bytes);
    uint32_t p, w;
    reduce_batch_plan(count, elem_bytes, p, w);
    store(path, p);
    store(workgroups, w);
    return GLU_OK;
}

glu_status glu_reduce_prepare_batch(glu_reduce reduce, size_t total, size_t num_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(reduce, "reduce"));
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    const size_t elem_bytes = data_type_size(reduce->type);
    BatchListsLayout layout;
    GLU_TRY(reserve_batch_lists(reduce->batch_lists, classes_of(elem_bytes), total, num_segments, layout));
    return reserve_partials(reduce, total, num_segments, layout, elem_bytes);
}

glu_status glu_reduce_run_batch_ptr(glu_reduce reduce, const void* data, void* out, size_t count, size_t num_partitions, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(reduce, "reduce"));
    if (num_partitions >= ((size_t) 1 << 31)) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_partitions %zu is not below 2^31", num_partitions);
    if (count && num_partitions > ((size_t) -1) / count) return fail(GLU_ERROR_INVALID_ARGUMENT, "count * num_partitions overflows");
    GLU_TRY(check_arrays(reduce, data, out, count * num_partitions, num_partitions));
    if (num_partitions == 0)
    {
        reduce->last_batch.reset();
        return GLU_OK;
    }
    BatchRunner r{{reduce, data, out, count, num_partitions, count * num_partitions, nullptr, pick_stream(stream)}};
    return dispatch_type(reduce->type, r);
}

glu_status glu_reduce_run_batch_offsets_ptr(glu_reduce reduce, const void* data, void* out, size_t total, const uint32_t* offsets,
                                            size_t num_segments, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(reduce, "reduce"));
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_arrays(reduce, data, out, num_segments ? total : 0, num_segments));
    GLU_TRY(check_batch_offsets(offsets, num_segments));
    if (num_segments == 0)
    {
        reduce->last_batch.reset();
        return GLU_OK;
    }
    BatchRunner r{{reduce, data, out, 0, num_segments, total, offsets, pick_stream(stream)}};
    return dispatch_type(reduce->type, r);
}

glu_status glu_reduce_read_batch(glu_reduce reduce, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(reduce, "reduce"));
    return reduce->last_batch.read(reduce->batch_lists, 3, wave_segments, block_segments, long_segments); // (the three short lists)
}

} // extern "C"
