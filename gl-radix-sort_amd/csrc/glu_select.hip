// glu_select.hip -- select of libglu_hip.so (select_kernels.hpp): glu_select_create, glu_select_destroy, glu_select_prepare,
// glu_select_run_ptr, glu_select_plan.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "glu_select_object.hpp"
#include "select_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(GLU_SELECT_EQ == SELECT_EQ && GLU_SELECT_NE == SELECT_NE && GLU_SELECT_LT == SELECT_LT && GLU_SELECT_LE == SELECT_LE &&
                  GLU_SELECT_GT == SELECT_GT && GLU_SELECT_GE == SELECT_GE && GLU_SELECT_OP_COUNT_ == SELECT_OPS_,
              "the header's comparisons are the kernels'");

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

} // extern "C"
