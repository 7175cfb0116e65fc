// glu_gather.hip -- gather and scatter of libglu_hip.so (gather_kernels.hpp): glu_gather_create, glu_gather_destroy,
// glu_gather_run_ptr, glu_gather_run_batch_ptr, glu_gather_run_batch_offsets_ptr, glu_gather_scatter_ptr, glu_gather_plan,
// glu_gather_last.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include "gather_kernels.hpp"
#include "glu_gather_object.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
enum Form
{
    FORM_GATHER,
    FORM_BATCH,
    FORM_SCATTER
};

// item_count and out_count: every uint32 index can name an entry, none needs more
glu_status check_table(size_t entries, const char* name)
{
    return entries <= kGatherMaxTable ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "%s must not exceed 2^32 (got %zu)", name, entries);
}

// the limits of batched top-k, whose rows these calls read
glu_status check_batch_sizes(size_t total, size_t num_segments, size_t k)
{
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_total(total));
    if (k && num_segments && (k > kGatherMaxCount || num_segments * k > kGatherMaxCount))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments * k must stay below 2^32 (got num_segments %zu, k %zu)", num_segments, k);
    return GLU_OK;
}

// One kernel over the streaming side (`stream_side`: `entries` items from there), or nothing where there is no entry.
template<uint32_t ITEM_BYTES>
glu_status launch(glu_gather gather, Form form, GatherArgs a, const void* stream_side, uint64_t entries, hipStream_t stream)
{
    using Cfg = GatherCfg<ITEM_BYTES>;
    using Piece = typename GatherPiece<Cfg::PIECE_BYTES>::type;
    const TileSpan<Piece> span = tile_span<Piece, Cfg::PACKS>(stream_side, entries * Cfg::PIECES);
    a.lo = span.lo;
    a.hi = span.hi;
    gather->last = {span.tiles, 1u};
    const dim3 grid(span.tiles), block(kGatherThreads);
    switch (form)
    {
    case FORM_GATHER: hipLaunchKernelGGL((gather_kernel<ITEM_BYTES, false>), grid, block, 0, stream, a); break;
    case FORM_BATCH: hipLaunchKernelGGL((gather_kernel<ITEM_BYTES, true>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((scatter_kernel<ITEM_BYTES>), grid, block, 0, stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

glu_status launch(glu_gather gather, Form form, const GatherArgs& a, const void* stream_side, uint64_t entries, uint32_t item_bytes,
                  void* stream)
{
    const hipStream_t st = pick_stream(stream);
    switch (item_bytes)
    {
    case 4: return launch<4>(gather, form, a, stream_side, entries, st);
    case 8: return launch<8>(gather, form, a, stream_side, entries, st);
    case 16: return launch<16>(gather, form, a, stream_side, entries, st);
    default: return launch<32>(gather, form, a, stream_side, entries, st);
    }
}

// the batched forms behind their size checks: `offsets` NULL for equal partitions of `count`
glu_status run_batch(glu_gather gather, const void* items, uint32_t item_bytes, size_t total, size_t count, const uint32_t* offsets,
                     size_t num_segments, const uint32_t* indices, size_t k, void* out, void* stream)
{
    const size_t entries = num_segments * k;
    if (!entries) // no segment or k == 0: no array is looked at
    {
        gather->last = {0u, 0u};
        return GLU_OK;
    }
    GLU_TRY(check_not_null(items, "items"));
    GLU_TRY(check_not_null(indices, "indices"));
    GLU_TRY(check_not_null(out, "out"));
    const char* to = bytes_text(item_align(item_bytes));
    GLU_TRY(check_aligned(items, item_align(item_bytes), "items", to));
    GLU_TRY(check_aligned(out, item_align(item_bytes), "out", to));
    GLU_TRY(check_aligned_4(indices, "indices"));
    GLU_TRY(check_disjoint({{out, entries * item_bytes, "out"}},
                           {{items, total * item_bytes, "items"}, {indices, entries * 4, "indices"}, {offsets, (num_segments + 1) * 4, "offsets"}}));
    GatherArgs a = {};
    a.items = items;
    a.indices = indices;
    a.out = out;
    a.offsets = offsets;
    a.rows = gather_make_rows((uint32_t) k, (uint32_t) count, (uint32_t) total, offsets != nullptr);
    return launch(gather, FORM_BATCH, a, out, entries, item_bytes, stream);
}
} // namespace

extern "C" {

glu_status glu_gather_plan(size_t count, uint32_t item_bytes, uint32_t* tile, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(check_item_bytes(item_bytes));
    GLU_TRY(check_below_2_32(count, "count"));
    const GatherPlan p = gather_plan(count, item_bytes);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    return GLU_OK;
}

glu_status glu_gather_create(glu_gather* out) { return create_object(out); }

glu_status glu_gather_destroy(glu_gather gather) { return destroy_object(gather); }

glu_status glu_gather_run_ptr(glu_gather gather, const void* items, size_t item_count, uint32_t item_bytes, const uint32_t* indices,
                              size_t count, void* out, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(gather, "gather"));
    GLU_TRY(check_item_bytes(item_bytes));
    GLU_TRY(check_below_2_32(count, "count"));
    GLU_TRY(check_table(item_count, "item_count"));
    if (!count || !item_count) // nothing can be fetched: no array is looked at
    {
        gather->last = {0u, 0u};
        return GLU_OK;
    }
    GLU_TRY(check_not_null(items, "items"));
    GLU_TRY(check_not_null(indices, "indices"));
    GLU_TRY(check_not_null(out, "out"));
    const char* to = bytes_text(item_align(item_bytes));
    GLU_TRY(check_aligned(items, item_align(item_bytes), "items", to));
    GLU_TRY(check_aligned(out, item_align(item_bytes), "out", to));
    GLU_TRY(check_aligned_4(indices, "indices"));
    GLU_TRY(check_disjoint({{out, count * item_bytes, "out"}}, {{items, item_count * item_bytes, "items"}, {indices, count * 4, "indices"}}));
    GatherArgs a = {};
    a.items = items;
    a.indices = indices;
    a.out = out;
    a.bound = item_count;
    return launch(gather, FORM_GATHER, a, out, count, item_bytes, stream);
}

glu_status glu_gather_run_batch_ptr(glu_gather gather, const void* items, uint32_t item_bytes, size_t count, size_t num_partitions,
                                    const uint32_t* indices, size_t k, void* out, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(gather, "gather"));
    GLU_TRY(check_item_bytes(item_bytes));
    if (count && num_partitions > ((size_t) -1) / count) return fail(GLU_ERROR_INVALID_ARGUMENT, "count * num_partitions overflows");
    GLU_TRY(check_batch_sizes(count * num_partitions, num_partitions, k));
    return run_batch(gather, items, item_bytes, count * num_partitions, count, nullptr, count ? num_partitions : 0, indices, k, out, stream);
}

glu_status glu_gather_run_batch_offsets_ptr(glu_gather gather, const void* items, uint32_t item_bytes, size_t total, const uint32_t* offsets,
                                            size_t num_segments, const uint32_t* indices, size_t k, void* out, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(gather, "gather"));
    GLU_TRY(check_item_bytes(item_bytes));
    GLU_TRY(check_batch_sizes(total, num_segments, k));
    if (total && num_segments && k)
    {
        GLU_TRY(check_not_null(offsets, "offsets"));
        GLU_TRY(check_aligned_4(offsets, "offsets"));
    }
    return run_batch(gather, items, item_bytes, total, 0, offsets, total ? num_segments : 0, indices, k, out, stream);
}

glu_status glu_gather_scatter_ptr(glu_gather gather, const void* items, uint32_t item_bytes, const uint32_t* indices, size_t count, void* out,
                                  size_t out_count, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(gather, "gather"));
    GLU_TRY(check_item_bytes(item_bytes));
    GLU_TRY(check_below_2_32(count, "count"));
    GLU_TRY(check_table(out_count, "out_count"));
    if (!count || !out_count) // nothing can be placed: no array is looked at
    {
        gather->last = {0u, 0u};
        return GLU_OK;
    }
    GLU_TRY(check_not_null(items, "items"));
    GLU_TRY(check_not_null(indices, "indices"));
    GLU_TRY(check_not_null(out, "out"));
    const char* to = bytes_text(item_align(item_bytes));
    GLU_TRY(check_aligned(items, item_align(item_bytes), "items", to));
    GLU_TRY(check_aligned(out, item_align(item_bytes), "out", to));
    GLU_TRY(check_aligned_4(indices, "indices"));
    GLU_TRY(check_disjoint({{out, out_count * item_bytes, "out"}}, {{items, count * item_bytes, "items"}, {indices, count * 4, "indices"}}));
    GatherArgs a = {};
    a.items = items;
    a.indices = indices;
    a.out = out;
    a.bound = out_count;
    return launch(gather, FORM_SCATTER, a, items, count, item_bytes, stream);
}

glu_status glu_gather_last(glu_gather gather, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(gather, "gather"));
    store(tiles, gather->last.tiles);
    store(kernels, gather->last.kernels);
    return GLU_OK;
}

} // extern "C"
