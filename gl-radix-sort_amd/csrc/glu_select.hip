// glu_select.hip -- select of libglu_hip.so (select_kernels.hpp): glu_select_create, glu_select_destroy, glu_select_prepare,
// glu_select_run_ptr, glu_select_plan; and the batched select (select_batch_kernels.hpp over select_batch_rank.hpp):
// glu_select_run_batch_ptr, glu_select_run_batch_offsets_ptr, glu_select_prepare_batch, glu_select_plan_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "glu_select_object.hpp"
#include "select_batch_kernels.hpp"
#include "select_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(GLU_SELECT_EQ == SELECT_EQ && GLU_SELECT_NE == SELECT_NE && GLU_SELECT_LT == SELECT_LT && GLU_SELECT_LE == SELECT_LE &&
                  GLU_SELECT_GT == SELECT_GT && GLU_SELECT_GE == SELECT_GE && GLU_SELECT_OP_COUNT_ == SELECT_OPS_,
              "the header's comparisons are the kernels'");
static_assert(GLU_SELECT_INDEX_GLOBAL == SELECT_INDEX_GLOBAL && GLU_SELECT_INDEX_LOCAL == SELECT_INDEX_LOCAL, "the header's index forms are the kernels'");

namespace
{
glu_status check_count(size_t count) { return check_tile_count(count, "select takes a count below 2^32"); }

// bytes of a stencil element, 0 for what is no stencil type
uint32_t stencil_bytes(int stencil_type)
{
    switch (stencil_type)
    {
    case GLU_DATA_TYPE_FLOAT:
    case GLU_DATA_TYPE_INT:
    case GLU_DATA_TYPE_UINT: return 4;
    case GLU_DATA_TYPE_DOUBLE: return 8;
    case GLU_SELECT_STENCIL_BYTE: return 1;
    default: return 0;
    }
}

glu_status check_stencil_type(int stencil_type)
{
    return stencil_bytes(stencil_type)
               ? GLU_OK
               : fail(GLU_ERROR_INVALID_ARGUMENT, "stencil_type must be FLOAT, DOUBLE, INT, UINT (0 .. 3) or GLU_SELECT_STENCIL_BYTE (12) (got %d)",
                      stencil_type);
}

struct Call
{
    glu_select_s* sel;
    const void* stencil;
    int op;
    const void* threshold;
    size_t count;
    const void* items;
    uint32_t item_bytes;
    void* out_items;
    uint32_t* out_indices;
    size_t max_out;
    uint32_t* num_selected;
    hipStream_t stream;
};

template<typename S, uint32_t ITEM_BYTES>
void launch_write(const Call& c, const SelectArgs<S>& a, const uint32_t* tile_counts, uint32_t grid)
{
    hipLaunchKernelGGL((select_write_kernel<S, ITEM_BYTES>), dim3(grid), dim3(kTileThreads), 0, c.stream, a, tile_counts, c.items, c.out_items,
                       c.out_indices, (uint32_t) c.max_out);
}

// Three kernels, whatever the stencil holds: the selected elements of every tile counted, the counts scanned by one workgroup,
// the selected elements written at their ranks.  The grids follow from `count` and the alignment of `stencil`, and whether the third
// kernel is enqueued at all from the output pointers and `max_out`: never from the data.
template<typename S>
glu_status run(const Call& c)
{
    SelectArgs<S> a;
    a.stencil = tile_span<S, SelectCfg<S>::PACKS>(c.stencil, c.count);
    S threshold = (S) 0; // (NULL: zero)
    if (c.threshold) memcpy(&threshold, c.threshold, sizeof(S));
    a.pred = make_select_pred<S>(c.op, threshold);
    const uint32_t tiles = a.stencil.tiles, grid = tile_grid(tiles);
    uint32_t* tile_counts = (uint32_t*) c.sel->tile_counts.ptr;
    hipLaunchKernelGGL((select_count_kernel<S>), dim3(grid), dim3(kTileThreads), 0, c.stream, a, tile_counts);
    HIP_TRY(hipGetLastError());
    GLU_TRY(launch_tile_count_scan(tile_counts, tiles, c.num_selected, c.stream));
    if (!tiles || !c.max_out || (!c.out_items && !c.out_indices)) return GLU_OK; // (nothing can be written: the call only counts)
    switch (c.items ? c.item_bytes : 0u)
    {
    case 0: launch_write<S, 0>(c, a, tile_counts, grid); break;
    case 4: launch_write<S, 4>(c, a, tile_counts, grid); break;
    case 8: launch_write<S, 8>(c, a, tile_counts, grid); break;
    case 16: launch_write<S, 16>(c, a, tile_counts, grid); break;
    default: launch_write<S, 32>(c, a, tile_counts, grid); break;
    }
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// ---- the batched call ---------------------------------------------------------------------------------------------------------
struct BatchCall
{
    Call c; // (count: the batch's total)
    const uint32_t* offsets; // nullptr: equal partitions of `partition`
    size_t partition, num_segments;
    int index_form;
    uint32_t* out_offsets;
};

glu_status reserve_batch(glu_select_s* sel, size_t total, uint32_t sb)
{
    return sel->batch.reserve(select_batch_scratch(total, sb, select_packs(sb)).bytes);
}

// kernels of a batched call with these outputs (the count scan among them); 0 where the call only clears
uint32_t batch_kernels(size_t total, size_t num_segments, bool offsets_out, bool compacts)
{
    if (!num_segments || !total) return 0;
    return 2u + (offsets_out ? 1u : 0u) + (compacts ? 1u : 0u);
}

template<uint32_t SB, uint32_t ITEM_BYTES>
void launch_batch_write(const BatchCall& b, const SelectBatchSegs& segs, uint64_t lo, uint32_t tiles, const SelectBatchScratchPtrs& p, uint32_t grid)
{
    const Call& c = b.c;
    if (b.index_form == GLU_SELECT_INDEX_LOCAL && c.out_indices)
        hipLaunchKernelGGL((select_batch_write_kernel<SB, ITEM_BYTES, true>), dim3(grid), dim3(kTileThreads), 0, c.stream, segs, lo, tiles, p, c.items,
                           c.out_items, c.out_indices, (uint32_t) c.max_out);
    else
        hipLaunchKernelGGL((select_batch_write_kernel<SB, ITEM_BYTES, false>), dim3(grid), dim3(kTileThreads), 0, c.stream, segs, lo, tiles, p, c.items,
                           c.out_items, c.out_indices, (uint32_t) c.max_out);
}

// At most four kernels: the count with its flag words, the count scan, a thread per boundary, the write from the flag words.  Which
// of the last two are enqueued follows from the output pointers and max_out, the grids from total, num_segments and the address
// of the stencil: never from the data.
template<typename S>
glu_status run_batch(const BatchCall& b)
{
    const Call& c = b.c;
    if (!b.num_segments || !c.count) // (nothing is selected: the count and every offset are zero)
    {
        HIP_TRY(hipMemsetAsync(c.num_selected, 0, sizeof(uint32_t), c.stream));
        if (b.num_segments && b.out_offsets) HIP_TRY(hipMemsetAsync(b.out_offsets, 0, (b.num_segments + 1) * sizeof(uint32_t), c.stream));
        return GLU_OK;
    }
    constexpr uint32_t SB = sizeof(S);
    SelectArgs<S> a;
    a.stencil = tile_span<S, SelectCfg<S>::PACKS>(c.stencil, c.count);
    S threshold = (S) 0; // (NULL: zero)
    if (c.threshold) memcpy(&threshold, c.threshold, sizeof(S));
    a.pred = make_select_pred<S>(c.op, threshold);
    const uint32_t tiles = a.stencil.tiles, grid = tile_grid(tiles);
    const SelectBatchScratch at = select_batch_scratch(c.count, SB, select_packs(SB));
    char* scratch = (char*) c.sel->batch.ptr;
    const SelectBatchScratchPtrs p = {(uint32_t*) (scratch + at.counts_at), (uint32_t*) (scratch + at.below_at), scratch + at.flags_at};
    const SelectBatchSegs segs = {b.offsets, (uint32_t) b.num_segments, (uint32_t) b.partition, (uint32_t) c.count};
    hipLaunchKernelGGL((select_batch_count_kernel<S>), dim3(grid), dim3(kTileThreads), 0, c.stream, a, segs, p);
    HIP_TRY(hipGetLastError());
    GLU_TRY(launch_tile_count_scan(p.tile_counts, tiles + 1, c.num_selected, c.stream));
    if (b.out_offsets)
    {
        const uint32_t blocks = (uint32_t) std::min<uint64_t>((b.num_segments + 1 + 255) / 256, cus() * 8u);
        hipLaunchKernelGGL((select_batch_offsets_kernel<SB>), dim3(blocks), dim3(256), 0, c.stream, segs, a.stencil.lo, tiles, p, b.out_offsets,
                           (uint32_t) c.max_out);
        HIP_TRY(hipGetLastError());
    }
    if (!c.max_out || (!c.out_items && !c.out_indices)) return GLU_OK; // (nothing can be written)
    switch (c.items ? c.item_bytes : 0u)
    {
    case 0: launch_batch_write<SB, 0>(b, segs, a.stencil.lo, tiles, p, grid); break;
    case 4: launch_batch_write<SB, 4>(b, segs, a.stencil.lo, tiles, p, grid); break;
    case 8: launch_batch_write<SB, 8>(b, segs, a.stencil.lo, tiles, p, grid); break;
    case 16: launch_batch_write<SB, 16>(b, segs, a.stencil.lo, tiles, p, grid); break;
    default: launch_batch_write<SB, 32>(b, segs, a.stencil.lo, tiles, p, grid); break;
    }
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

glu_status check_index_form(int index_form)
{
    return index_form == GLU_SELECT_INDEX_GLOBAL || index_form == GLU_SELECT_INDEX_LOCAL
               ? GLU_OK
               : fail(GLU_ERROR_INVALID_ARGUMENT, "index_form must be GLU_SELECT_INDEX_GLOBAL (0) or GLU_SELECT_INDEX_LOCAL (1) (got %d)", index_form);
}

// The checks of the single call in its order, and between them those of the segments and of out_offsets.
glu_status check_and_run_batch(glu_select_s* select, const void* stencil, int stencil_type, int op, const void* threshold, size_t partition,
                               size_t total, const uint32_t* offsets, bool with_offsets, size_t num_segments, const void* items,
                               uint32_t item_bytes, void* out_items, uint32_t* out_indices, int index_form, size_t max_out,
                               uint32_t* out_offsets, uint32_t* num_selected, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(select, "select"));
    GLU_TRY(check_stencil_type(stencil_type));
    if (op < 0 || op >= GLU_SELECT_OP_COUNT_) return fail(GLU_ERROR_INVALID_ARGUMENT, "op must be one of GLU_SELECT_EQ .. GLU_SELECT_GE (got %d)", op);
    GLU_TRY(check_index_form(index_form));
    GLU_TRY(check_batch_segments(num_segments));
    if (!with_offsets)
    {
        GLU_TRY(check_count(partition));
        total = partition * num_segments; // (below 2^56)
    }
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_below_2_32(max_out, "max_out"));
    if (total && !stencil) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid stencil buffer");
    if (!num_selected) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_selected pointer");
    if (!items != !out_items) return fail(GLU_ERROR_INVALID_ARGUMENT, "items and out_items must both be given or both be NULL");
    if (items) GLU_TRY(check_item_bytes(item_bytes));
    if (with_offsets) GLU_TRY(check_batch_offsets(offsets, num_segments));
    const size_t sb = stencil_bytes(stencil_type), ib = items ? item_bytes : 0;
    GLU_TRY(check_aligned(stencil, sb, "stencil", "its element size"));
    GLU_TRY(check_items_aligned(items, out_items, item_bytes, "min(item_bytes, 16)"));
    GLU_TRY(check_aligned_4(out_indices, "out_indices"));
    GLU_TRY(check_aligned_4(out_offsets, "out_offsets"));
    GLU_TRY(check_aligned_4(num_selected, "num_selected"));
    const size_t written = std::min(total, max_out), bounds = num_segments ? (num_segments + 1) * sizeof(uint32_t) : 0;
    const Array in_offsets = {with_offsets ? offsets : nullptr, bounds, "offsets"}, new_offsets = {out_offsets, bounds, "out_offsets"};
    const Array new_items = {out_items, written * ib, "out_items"}, new_indices = {out_indices, written * sizeof(uint32_t), "out_indices"},
                count_out = {num_selected, sizeof(uint32_t), "num_selected"};
    GLU_TRY(check_disjoint({new_items, new_indices, count_out, new_offsets},
                           {{stencil, total * sb, "stencil"}, {items, total * ib, "items"}, in_offsets}));
    GLU_TRY(check_disjoint({new_offsets}, {new_items, new_indices, count_out}));
    GLU_TRY(reserve_batch(select, total, (uint32_t) sb));
    const BatchCall b = {{select, stencil, op, threshold, total, items, item_bytes, out_items, out_indices, max_out, num_selected, pick_stream(stream)},
                         with_offsets ? offsets : nullptr, partition, num_segments, index_form, out_offsets};
    switch (stencil_type)
    {
    case GLU_DATA_TYPE_FLOAT: return run_batch<float>(b);
    case GLU_DATA_TYPE_DOUBLE: return run_batch<double>(b);
    case GLU_DATA_TYPE_INT: return run_batch<int32_t>(b);
    case GLU_DATA_TYPE_UINT: return run_batch<uint32_t>(b);
    default: return run_batch<uint8_t>(b);
    }
}
} // namespace

extern "C" {

glu_status glu_select_plan(size_t count, int stencil_type, uint32_t* tile, uint32_t* tiles, uint32_t* scan_rounds)
{
    GLU_TRY(check_stencil_type(stencil_type));
    GLU_TRY(check_count(count));
    const uint32_t sb = stencil_bytes(stencil_type);
    const TilePlan p = tile_plan(count, sb, select_packs(sb));
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(scan_rounds, p.scan_rounds);
    return GLU_OK;
}

glu_status glu_select_create(glu_select* out) { return create_object(out); }

glu_status glu_select_destroy(glu_select select) { return destroy_object(select); }

glu_status glu_select_prepare(glu_select select, size_t count, int stencil_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(select, "select"));
    GLU_TRY(check_stencil_type(stencil_type));
    GLU_TRY(check_count(count));
    const uint32_t sb = stencil_bytes(stencil_type);
    return select->tile_counts.reserve(count, sb, select_packs(sb));
}

glu_status glu_select_run_ptr(glu_select select, const void* stencil, int stencil_type, int op, const void* threshold, size_t count,
                              const void* items, uint32_t item_bytes, void* out_items, uint32_t* out_indices, size_t max_out,
                              uint32_t* num_selected, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(select, "select"));
    GLU_TRY(check_stencil_type(stencil_type));
    if (op < 0 || op >= GLU_SELECT_OP_COUNT_) return fail(GLU_ERROR_INVALID_ARGUMENT, "op must be one of GLU_SELECT_EQ .. GLU_SELECT_GE (got %d)", op);
    GLU_TRY(check_count(count));
    GLU_TRY(check_below_2_32(max_out, "max_out"));
    if (count && !stencil) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid stencil buffer");
    if (!num_selected) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_selected pointer");
    if (!items != !out_items) return fail(GLU_ERROR_INVALID_ARGUMENT, "items and out_items must both be given or both be NULL");
    if (items) GLU_TRY(check_item_bytes(item_bytes));
    const size_t sb = stencil_bytes(stencil_type), ib = items ? item_bytes : 0;
    GLU_TRY(check_aligned(stencil, sb, "stencil", "its element size"));
    GLU_TRY(check_items_aligned(items, out_items, item_bytes, "min(item_bytes, 16)"));
    GLU_TRY(check_aligned_4(out_indices, "out_indices"));
    GLU_TRY(check_aligned_4(num_selected, "num_selected"));
    // (no more than min(count, max_out) entries of an output array can be written; the outputs are not held against each other)
    const size_t written = std::min(count, max_out);
    GLU_TRY(check_disjoint({{out_items, written * ib, "out_items"}, {out_indices, written * sizeof(uint32_t), "out_indices"},
                            {num_selected, sizeof(uint32_t), "num_selected"}},
                           {{stencil, count * sb, "stencil"}, {items, count * ib, "items"}}));
    GLU_TRY(select->tile_counts.reserve(count, (uint32_t) sb, select_packs((uint32_t) sb)));
    const Call c{select, stencil, op, threshold, count, items, item_bytes, out_items, out_indices, max_out, num_selected, pick_stream(stream)};
    switch (stencil_type)
    {
    case GLU_DATA_TYPE_FLOAT: return run<float>(c);
    case GLU_DATA_TYPE_DOUBLE: return run<double>(c);
    case GLU_DATA_TYPE_INT: return run<int32_t>(c);
    case GLU_DATA_TYPE_UINT: return run<uint32_t>(c);
    default: return run<uint8_t>(c);
    }
}

glu_status glu_select_plan_batch(size_t total, size_t num_segments, int stencil_type, int index_form, uint32_t* tile, uint32_t* tiles,
                                 uint32_t* scan_rounds, uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_stencil_type(stencil_type));
    GLU_TRY(check_index_form(index_form));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_total(total));
    const uint32_t sb = stencil_bytes(stencil_type);
    const TilePlan p = tile_plan(total, sb, select_packs(sb));
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(scan_rounds, total ? (p.tiles + 1 + kTileScanRound - 1) / kTileScanRound : 0u); // (tiles + 1 counts: the last becomes the total)
    store(kernels, batch_kernels(total, num_segments, true, true));
    store(scratch_bytes, select_batch_scratch(total, sb, select_packs(sb)).bytes);
    return GLU_OK;
}

glu_status glu_select_prepare_batch(glu_select select, size_t total, size_t num_segments, int stencil_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(select, "select"));
    GLU_TRY(check_stencil_type(stencil_type));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_total(total));
    return reserve_batch(select, total, stencil_bytes(stencil_type));
}

glu_status glu_select_run_batch_ptr(glu_select select, const void* stencil, int stencil_type, int op, const void* threshold, size_t count,
                                    size_t num_partitions, const void* items, uint32_t item_bytes, void* out_items, uint32_t* out_indices,
                                    int index_form, size_t max_out, uint32_t* out_offsets, uint32_t* num_selected, void* stream)
{
    return check_and_run_batch(select, stencil, stencil_type, op, threshold, count, 0, nullptr, false, num_partitions, items, item_bytes, out_items,
                               out_indices, index_form, max_out, out_offsets, num_selected, stream);
}

glu_status glu_select_run_batch_offsets_ptr(glu_select select, const void* stencil, int stencil_type, int op, const void* threshold, size_t total,
                                            const uint32_t* offsets, size_t num_segments, const void* items, uint32_t item_bytes,
                                            void* out_items, uint32_t* out_indices, int index_form, size_t max_out, uint32_t* out_offsets,
                                            uint32_t* num_selected, void* stream)
{
    return check_and_run_batch(select, stencil, stencil_type, op, threshold, 0, total, offsets, true, num_segments, items, item_bytes, out_items,
                               out_indices, index_form, max_out, out_offsets, num_selected, stream);
}

} // extern "C"
