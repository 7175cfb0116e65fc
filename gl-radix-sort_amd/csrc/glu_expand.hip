// glu_expand.hip -- expand of libglu_hip.so (expand_kernels.hpp): glu_expand_create, glu_expand_destroy, glu_expand_prepare,
// glu_expand_run_ptr, glu_expand_plan, glu_expand_last.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include "expand_kernels.hpp"
#include "glu_expand_object.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// (each count first: their sum must not wrap)
glu_status check_sizes(size_t total, size_t num_segments)
{
    if (num_segments > kExpandMaxSegments)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "expand takes num_segments up to 2^24 (got %zu)", num_segments);
    if (total > kExpandMaxMerged || (uint64_t) total + num_segments + 1 > kExpandMaxMerged)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "expand takes total + num_segments + 1 below 2^32 (got total %zu, num_segments %zu)", total,
                    num_segments);
    return GLU_OK;
}

template<uint32_t ITEM_WORDS>
glu_status launch(const ExpandArgs& e, hipStream_t stream)
{
    hipLaunchKernelGGL(expand_partition_kernel, dim3(e.tiles / kExpandThreads + 1), dim3(kExpandThreads), 0, stream, e);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((expand_tile_kernel<ITEM_WORDS>), dim3(e.tiles), dim3(kExpandThreads), 0, stream, e);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}
} // namespace

extern "C" {

glu_status glu_expand_plan(size_t total, size_t num_segments, uint32_t* tile, uint32_t* tiles, uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_sizes(total, num_segments));
    const ExpandPlan p = expand_plan(total, num_segments);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_expand_create(glu_expand* out) { return create_object(out); }

glu_status glu_expand_destroy(glu_expand expand) { return destroy_object(expand); }

glu_status glu_expand_prepare(glu_expand expand, size_t total, size_t num_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(expand, "expand"));
    GLU_TRY(check_sizes(total, num_segments));
    return expand->split.reserve(expand_plan(total, num_segments).scratch_bytes);
}

glu_status glu_expand_run_ptr(glu_expand expand, const uint32_t* offsets, size_t num_segments, size_t total, const void* items,
                              uint32_t item_bytes, void* out_items, uint32_t* out_segments, uint32_t* out_ranks, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(expand, "expand"));
    GLU_TRY(check_sizes(total, num_segments));
    ExpandPlan p = expand_plan(total, num_segments);
    if (!p.kernels) // no position or no segment: no array is looked at
    {
        expand->last = {0u, 0u};
        return GLU_OK;
    }
    if (!offsets) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid offsets buffer");
    if ((items != nullptr) != (out_items != nullptr))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "items and out_items must be both NULL (no gather) or both non-NULL");
    if (items) GLU_TRY(check_item_bytes(item_bytes));
    if (!items) item_bytes = 0;
    GLU_TRY(check_aligned_4(offsets, "offsets"));
    GLU_TRY(check_aligned_4(out_segments, "out_segments"));
    GLU_TRY(check_aligned_4(out_ranks, "out_ranks"));
    GLU_TRY(check_items_aligned(items, out_items, item_bytes, bytes_text(item_align(item_bytes))));
    // an output against every array behind it: the other outputs and the inputs
    GLU_TRY(check_disjoint({{out_segments, total * 4, "out_segments"}, {out_ranks, total * 4, "out_ranks"}, {out_items, total * item_bytes, "out_items"}},
                           {{offsets, (num_segments + 1) * 4, "offsets"}, {items, num_segments * item_bytes, "items"}}, kOutputsBeforeInputs));

    if (!out_segments && !out_ranks && !out_items) // nothing asked for
    {
        expand->last = {0u, 0u};
        return GLU_OK;
    }
    expand->last = {p.tiles, p.kernels};
    GLU_TRY(expand->split.reserve(p.scratch_bytes));
    ExpandArgs e = {};
    e.offsets = offsets;
    e.items = items;
    e.out_items = out_items;
    e.out_segments = out_segments;
    e.out_ranks = out_ranks;
    e.na = (uint32_t) num_segments + 1u;
    e.nb = (uint32_t) total;
    e.tiles = p.tiles;
    e.split = (uint32_t*) expand->split.ptr;
    const hipStream_t st = pick_stream(stream);
    switch (item_bytes)
    {
    case 4: return launch<1>(e, st);
    case 8: return launch<2>(e, st);
    case 16: return launch<4>(e, st);
    case 32: return launch<8>(e, st);
    default: return launch<0>(e, st);
    }
}

glu_status glu_expand_last(glu_expand expand, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(expand, "expand"));
    store(tiles, expand->last.tiles);
    store(kernels, expand->last.kernels);
    return GLU_OK;
}

} // extern "C"
