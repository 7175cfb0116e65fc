// glu_merge.hip -- merge of libglu_hip.so (merge_kernels.hpp): glu_merge_create, glu_merge_destroy, glu_merge_prepare,
// glu_merge_run_ptr, glu_merge_plan, glu_merge_last, and the batched merge (merge_batch_kernels.hpp): glu_merge_prepare_batch,
// glu_merge_run_batch_offsets_ptr, glu_merge_run_batch_ptr, glu_merge_plan_batch; and the set operations on merge's tiles (set_ops_kernels.hpp):
// glu_set_ops_create, glu_set_ops_destroy, glu_set_ops_prepare, glu_set_ops_run_ptr, glu_set_ops_plan, glu_set_ops_last, and the batched
// set operations (set_ops_batch_kernels.hpp): glu_set_ops_prepare_batch, glu_set_ops_run_batch_offsets_ptr, glu_set_ops_run_batch_ptr,
// glu_set_ops_plan_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "glu_batch_host.hpp"
#include "glu_merge_object.hpp"
#include "glu_set_ops_object.hpp"
#include "merge_batch_kernels.hpp"
#include "merge_kernels.hpp"
#include "set_ops_batch_kernels.hpp"
#include "set_ops_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(GLU_SET_UNION == kSetUnion && GLU_SET_INTERSECTION == kSetIntersection && GLU_SET_DIFFERENCE == kSetDifference &&
                  GLU_SET_SYMMETRIC_DIFFERENCE == kSetSymmetricDifference && GLU_SET_OP_COUNT_ == kSetOpCount,
              "the header's operations are the kernels'");

namespace
{
// (each count first: their sum must not wrap)
glu_status check_total(size_t a_count, size_t b_count)
{
    if (a_count > kMergeMaxTotal || b_count > kMergeMaxTotal || (uint64_t) a_count + (uint64_t) b_count > kMergeMaxTotal)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "merge takes a_count + b_count below 2^32 (got %zu + %zu)", a_count, b_count);
    return GLU_OK;
}

template<typename K>
glu_status launch(const MergeArgs<K>& m, const MergePlan& p, bool with_vals, hipStream_t stream)
{
    hipLaunchKernelGGL((merge_partition_kernel<K>), dim3(p.tiles / kMergeThreads + 1), dim3(kMergeThreads), 0, stream, m, p.tile);
    HIP_TRY(hipGetLastError());
    if (with_vals)
        hipLaunchKernelGGL((merge_tile_kernel<K, true>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    else
        hipLaunchKernelGGL((merge_tile_kernel<K, false>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

template<typename K>
glu_status run(glu_merge_s* s, const void* a_keys, const uint32_t* a_vals, size_t a_count, const void* b_keys, const uint32_t* b_vals,
               size_t b_count, void* out_keys, uint32_t* out_vals, int key_type, const MergePlan& p, hipStream_t stream)
{
    MergeArgs<K> m = {};
    m.a_keys = (const K*) a_keys;
    m.b_keys = (const K*) b_keys;
    m.a_vals = a_vals;
    m.b_vals = b_vals;
    m.out_keys = (K*) out_keys;
    m.out_vals = out_vals;
    m.na = (uint32_t) a_count;
    m.nb = (uint32_t) b_count;
    m.xf = key_xf_of(key_type);
    m.tiles = p.tiles;
    m.split = (uint32_t*) s->split.ptr;
    return launch<K>(m, p, out_vals != nullptr, stream);
}

// ---- the batched merge
struct BatchCall
{
    const void *a_keys, *b_keys;
    const uint32_t *a_vals, *b_vals;
    const uint32_t *a_offsets, *b_offsets; // NULL: equal partitions of a_len and b_len
    size_t a_len, b_len, a_total, b_total, num_segments;
    void* out_keys;
    uint32_t *out_vals, *out_offsets;
    int key_type;
    void* stream;
};

template<typename K>
glu_status run_batch(glu_merge_s* s, const BatchCall& c, const MergePlan& p, hipStream_t stream)
{
    MergeBatchArgs<K> m = {};
    m.a_keys = (const K*) c.a_keys;
    m.b_keys = (const K*) c.b_keys;
    m.a_vals = c.a_vals;
    m.b_vals = c.b_vals;
    m.out_keys = (K*) c.out_keys;
    m.out_vals = c.out_vals;
    m.a_offsets = c.a_offsets;
    m.b_offsets = c.b_offsets;
    m.a_len = (uint32_t) c.a_len;
    m.b_len = (uint32_t) c.b_len;
    m.a_total = (uint32_t) c.a_total;
    m.b_total = (uint32_t) c.b_total;
    m.num_segments = (uint32_t) c.num_segments;
    m.xf = key_xf_of(c.key_type);
    m.tiles = p.tiles;
    m.seg_steps = merge_steps(m.num_segments - 1u);
    m.split_steps = merge_steps(std::min(m.a_total, m.b_total));
    m.bounds = (MergeBatchBoundary*) s->split.ptr;
    m.out_offsets = c.out_offsets;
    // one thread per tile boundary and per out_offsets entry
    const uint32_t threads = std::max<uint32_t>(p.tiles, c.out_offsets ? m.num_segments : 0u);
    hipLaunchKernelGGL((merge_batch_partition_kernel<K>), dim3(threads / kMergeThreads + 1), dim3(kMergeThreads), 0, stream, m, p.tile);
    HIP_TRY(hipGetLastError());
    if (!p.tiles) return GLU_OK;
    if (c.out_vals)
        hipLaunchKernelGGL((merge_batch_tile_kernel<K, true>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    else
        hipLaunchKernelGGL((merge_batch_tile_kernel<K, false>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// Both forms of the batched call behind their own checks of the segments' shape.
glu_status merge_batch(glu_merge merge, BatchCall c)
{
    GLU_TRY(check_total(c.a_total, c.b_total));
    const uint32_t kb = key_bytes_of(c.key_type);
    const size_t total = c.a_total + c.b_total, words = c.num_segments + 1;
    // an array of no elements is not looked at
    if (!c.a_total) c.a_keys = nullptr, c.a_vals = nullptr;
    if (!c.b_total) c.b_keys = nullptr, c.b_vals = nullptr;
    if (!total) c.out_keys = nullptr, c.out_vals = nullptr;
    if (c.a_total && !c.a_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid a_keys buffer");
    if (c.b_total && !c.b_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid b_keys buffer");
    if (total && !c.out_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid out_keys buffer");
    const bool with_vals = c.out_vals != nullptr;
    if ((c.a_total && (c.a_vals != nullptr) != with_vals) || (c.b_total && (c.b_vals != nullptr) != with_vals))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "a_vals, b_vals and out_vals must be all NULL (keys only) or all non-NULL");
    GLU_TRY(check_aligned(c.a_keys, kb, "a_keys", "the key size"));
    GLU_TRY(check_aligned(c.b_keys, kb, "b_keys", "the key size"));
    GLU_TRY(check_aligned(c.out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(c.a_vals, "a_vals"));
    GLU_TRY(check_aligned_4(c.b_vals, "b_vals"));
    GLU_TRY(check_aligned_4(c.out_vals, "out_vals"));
    GLU_TRY(check_aligned_4(c.out_offsets, "out_offsets"));
    GLU_TRY(check_disjoint({{c.out_keys, total * kb, "out_keys"}, {c.out_vals, total * 4, "out_vals"}, {c.out_offsets, words * 4, "out_offsets"}},
                           {{c.a_keys, c.a_total * kb, "a_keys"},
                            {c.b_keys, c.b_total * kb, "b_keys"},
                            {c.a_vals, c.a_total * 4, "a_vals"},
                            {c.b_vals, c.b_total * 4, "b_vals"},
                            {c.a_offsets, words * 4, "a_offsets"},
                            {c.b_offsets, words * 4, "b_offsets"}},
                           kOutputsAfterInputs));

    const MergePlan p = merge_batch_plan(total, c.num_segments, kb, with_vals);
    merge->last = {p.tiles, p.kernels};
    const hipStream_t st = pick_stream(c.stream);
    if (!c.num_segments) // nothing to merge: out_offsets[0] = 0
    {
        if (c.out_offsets) HIP_TRY(hipMemsetAsync(c.out_offsets, 0, sizeof(uint32_t), st));
        return GLU_OK;
    }
    GLU_TRY(merge->split.reserve(p.scratch_bytes));
    return kb == 8 ? run_batch<uint64_t>(merge, c, p, st) : run_batch<uint32_t>(merge, c, p, st);
}

// ---- set operations
glu_status check_set_total(size_t a_count, size_t b_count)
{
    if (a_count > kSetOpsMaxTotal || b_count > kSetOpsMaxTotal || (uint64_t) a_count + (uint64_t) b_count > kSetOpsMaxTotal)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "set operations take a_count + b_count below 2^32 (got %zu + %zu)", a_count, b_count);
    return GLU_OK;
}

struct SetCall
{
    glu_set_ops_s* s;
    int op;
    const void *a_keys, *b_keys;
    const uint32_t *a_vals, *b_vals;
    size_t a_count, b_count;
    void* out_keys;
    uint32_t* out_vals;
    size_t room; // min(max_out, the operation's bound); 0: the call only counts
    uint32_t* num_out;
    int key_type;
    hipStream_t stream;
};

// Bounds, count, scan and (where something may be written) write.  The grids follow from the counts: never from the data.
template<typename K>
glu_status set_run(const SetCall& c, const SetOpsPlan& p, bool with_arrays)
{
    SetOpsArgs<K> m = {};
    m.a_keys = (const K*) c.a_keys;
    m.b_keys = (const K*) c.b_keys;
    m.a_vals = c.a_vals;
    m.b_vals = c.b_vals;
    m.out_keys = (K*) c.out_keys;
    m.out_vals = c.out_vals;
    m.na = (uint32_t) c.a_count;
    m.nb = (uint32_t) c.b_count;
    m.xf = key_xf_of(c.key_type);
    m.op = (uint32_t) c.op;
    m.tiles = p.tiles;
    m.room = (uint32_t) c.room;
    m.bounds = (SetBounds*) c.s->scratch.ptr;
    m.tile_counts = p.tiles ? (uint32_t*) (m.bounds + ((size_t) p.tiles + 1)) : nullptr;
    const uint32_t most = set_ops_total(kSetOpsMaxTotal, set_op_bound(m.op, m.na, m.nb));
    if (p.tiles)
    {
        hipLaunchKernelGGL((set_ops_bounds_kernel<K>), dim3(p.tiles / kMergeThreads + 1), dim3(kMergeThreads), 0, c.stream, m, p.tile);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((set_ops_count_kernel<K>), dim3(p.tiles), dim3(kMergeThreads), 0, c.stream, m);
        HIP_TRY(hipGetLastError());
    }
    GLU_TRY(launch_tile_count_scan(m.tile_counts, p.tiles, c.num_out, c.stream, most));
    if (!p.tiles || !with_arrays) return GLU_OK;
    if (c.out_vals)
        hipLaunchKernelGGL((set_ops_write_kernel<K, true>), dim3(p.tiles), dim3(kMergeThreads), 0, c.stream, m);
    else
        hipLaunchKernelGGL((set_ops_write_kernel<K, false>), dim3(p.tiles), dim3(kMergeThreads), 0, c.stream, m);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}
// ---- the batched set operations
struct SetBatchCall
{
    int op;
    const void *a_keys, *b_keys;
    const uint32_t *a_vals, *b_vals;
    const uint32_t *a_offsets, *b_offsets; // NULL: equal partitions of a_len and b_len
    size_t a_len, b_len, a_total, b_total, num_segments;
    void* out_keys;
    uint32_t* out_vals;
    size_t max_out;
    uint32_t *out_offsets, *num_out;
    int key_type;
    void* stream;
};

// Bounds, count, scan, offsets (where asked for) and write (where something may be written).  The grids follow from the host-known
// totals and the number of segments: never from the data.
template<typename K>
glu_status set_run_batch(glu_set_ops_s* s, const SetBatchCall& c, const SetOpsPlan& p, size_t room, bool with_arrays, hipStream_t stream)
{
    SetOpsBatchArgs<K> m = {};
    m.a_keys = (const K*) c.a_keys;
    m.b_keys = (const K*) c.b_keys;
    m.a_vals = c.a_vals;
    m.b_vals = c.b_vals;
    m.out_keys = (K*) c.out_keys;
    m.out_vals = c.out_vals;
    m.a_offsets = c.a_offsets;
    m.b_offsets = c.b_offsets;
    m.a_len = (uint32_t) c.a_len;
    m.b_len = (uint32_t) c.b_len;
    m.a_total = (uint32_t) c.a_total;
    m.b_total = (uint32_t) c.b_total;
    m.num_segments = (uint32_t) c.num_segments;
    m.xf = key_xf_of(c.key_type);
    m.op = (uint32_t) c.op;
    m.tiles = p.tiles;
    m.seg_steps = merge_steps(m.num_segments - 1u);
    m.split_steps = merge_steps(std::min(m.a_total, m.b_total));
    const uint32_t most = set_ops_total(kSetOpsMaxTotal, set_op_bound(m.op, m.a_total, m.b_total));
    m.room = (uint32_t) room;
    m.limit = with_arrays ? m.room : most;
    m.bounds = (SetBatchBounds*) s->scratch.ptr;
    m.tile_counts = p.tiles ? (uint32_t*) (m.bounds + ((size_t) p.tiles + 1)) : nullptr;
    m.words = (p.tiles && (with_arrays || c.out_offsets)) ? m.tile_counts + p.tiles : nullptr;
    m.out_offsets = c.out_offsets;
    m.num_out = c.num_out;
    if (p.tiles)
    {
        hipLaunchKernelGGL((set_batch_bounds_kernel<K>), dim3(p.tiles / kMergeThreads + 1), dim3(kMergeThreads), 0, stream, m, p.tile);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((set_batch_count_kernel<K>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
        HIP_TRY(hipGetLastError());
    }
    GLU_TRY(launch_tile_count_scan(m.tile_counts, p.tiles, c.num_out, stream, most));
    if (c.out_offsets) // one thread per entry
    {
        hipLaunchKernelGGL((set_batch_offsets_kernel<K>), dim3(m.num_segments / kMergeThreads + 1), dim3(kMergeThreads), 0, stream, m, p.tile,
                           merge_items(sizeof(K), true));
        HIP_TRY(hipGetLastError());
    }
    if (!p.tiles || !with_arrays) return GLU_OK;
    if (c.out_vals)
        hipLaunchKernelGGL((set_batch_write_kernel<K, true>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    else
        hipLaunchKernelGGL((set_batch_write_kernel<K, false>), dim3(p.tiles), dim3(kMergeThreads), 0, stream, m);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// Both forms of the batched call behind their own checks of the segments' shape.
glu_status set_ops_batch(glu_set_ops set_ops, SetBatchCall c)
{
    if (c.op < 0 || c.op >= GLU_SET_OP_COUNT_)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "op must be one of GLU_SET_UNION .. GLU_SET_SYMMETRIC_DIFFERENCE (got %d)", c.op);
    GLU_TRY(check_set_total(c.a_total, c.b_total));
    GLU_TRY(check_below_2_32(c.max_out, "max_out"));
    const uint32_t kb = key_bytes_of(c.key_type);
    const size_t total = c.a_total + c.b_total, words = c.num_segments + 1;
    // an array of no elements is not looked at
    if (!c.a_total) c.a_keys = nullptr, c.a_vals = nullptr;
    if (!c.b_total) c.b_keys = nullptr, c.b_vals = nullptr;
    if (c.a_total && !c.a_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid a_keys buffer");
    if (c.b_total && !c.b_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid b_keys buffer");
    if (!c.num_out) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_out pointer");
    const bool with_arrays = c.out_keys != nullptr && c.max_out != 0; // (else the call only counts)
    if (c.out_vals && !with_arrays)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "out_vals needs out_keys and max_out > 0 (a call that only counts takes neither)");
    const bool with_vals = c.out_vals != nullptr;
    if (c.a_total && (c.a_vals != nullptr) != with_vals)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "a_vals and out_vals must both be given or both be NULL");
    // B's values are read exactly where its elements can be written
    const bool b_written = with_vals && set_op_keeps_b((uint32_t) c.op) && c.b_total;
    if (b_written && !c.b_vals) return fail(GLU_ERROR_INVALID_ARGUMENT, "b_vals is required: the operation can write elements of B");
    if (!b_written) c.b_vals = nullptr;
    GLU_TRY(check_aligned(c.a_keys, kb, "a_keys", "the key size"));
    GLU_TRY(check_aligned(c.b_keys, kb, "b_keys", "the key size"));
    GLU_TRY(check_aligned(c.out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(c.a_vals, "a_vals"));
    GLU_TRY(check_aligned_4(c.b_vals, "b_vals"));
    GLU_TRY(check_aligned_4(c.out_vals, "out_vals"));
    GLU_TRY(check_aligned_4(c.out_offsets, "out_offsets"));
    GLU_TRY(check_aligned_4(c.num_out, "num_out"));
    // (no more than min(bound, max_out) entries of an output array can be written; the bound is the host-known totals')
    const size_t room = with_arrays ? (size_t) std::min<uint64_t>(set_op_bound((uint32_t) c.op, c.a_total, c.b_total), c.max_out) : 0;
    GLU_TRY(check_disjoint({{c.out_keys, room * kb, "out_keys"},
                            {c.out_vals, room * 4, "out_vals"},
                            {c.out_offsets, words * 4, "out_offsets"},
                            {c.num_out, sizeof(uint32_t), "num_out"}},
                           {{c.a_keys, c.a_total * kb, "a_keys"},
                            {c.b_keys, c.b_total * kb, "b_keys"},
                            {c.a_vals, c.a_total * 4, "a_vals"},
                            {c.b_vals, c.b_total * 4, "b_vals"},
                            {c.a_offsets, words * 4, "a_offsets"},
                            {c.b_offsets, words * 4, "b_offsets"}},
                           kOutputsAfterInputs));

    const SetOpsPlan p = set_ops_batch_plan(total, c.num_segments, kb, with_arrays, c.out_offsets != nullptr);
    GLU_TRY(set_ops->scratch.reserve(p.scratch_bytes));
    set_ops->last = {p.tiles, p.kernels};
    const hipStream_t st = pick_stream(c.stream);
    if (!c.num_segments) // nothing to look at: the scan alone writes *num_out = 0; out_offsets[0] = 0
    {
        if (c.out_offsets) HIP_TRY(hipMemsetAsync(c.out_offsets, 0, sizeof(uint32_t), st));
        return launch_tile_count_scan(nullptr, 0, c.num_out, st, 0u);
    }
    return kb == 8 ? set_run_batch<uint64_t>(set_ops, c, p, room, with_arrays, st) : set_run_batch<uint32_t>(set_ops, c, p, room, with_arrays, st);
}
} // namespace

extern "C" {

glu_status glu_merge_plan(size_t a_count, size_t b_count, glu_key_type key_type, int with_vals, uint32_t* tile, uint32_t* tiles,
                          uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_total(a_count, b_count));
    const MergePlan p = merge_plan((uint64_t) a_count + b_count, key_bytes_of((int) key_type), with_vals != 0);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_merge_create(glu_merge* out) { return create_object(out); }

glu_status glu_merge_destroy(glu_merge merge) { return destroy_object(merge); }

glu_status glu_merge_prepare(glu_merge merge, size_t total_count, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_total(total_count, 0));
    // (the tile is the same with and without values)
    return merge->split.reserve(merge_plan(total_count, key_bytes_of((int) key_type), true).scratch_bytes);
}

glu_status glu_merge_run_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, size_t a_count, const void* b_keys,
                             const uint32_t* b_vals, size_t b_count, void* out_keys, uint32_t* out_vals, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_total(a_count, b_count));
    const uint32_t kb = key_bytes_of((int) key_type);
    const size_t total = a_count + b_count;
    // a side of no elements is not looked at
    if (!a_count) a_keys = nullptr, a_vals = nullptr;
    if (!b_count) b_keys = nullptr, b_vals = nullptr;
    if (!total) out_keys = nullptr, out_vals = nullptr;
    if (a_count && !a_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid a_keys buffer");
    if (b_count && !b_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid b_keys buffer");
    if (total && !out_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid out_keys buffer");
    const bool with_vals = out_vals != nullptr;
    if ((a_count && (a_vals != nullptr) != with_vals) || (b_count && (b_vals != nullptr) != with_vals))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "a_vals, b_vals and out_vals must be all NULL (keys only) or all non-NULL");
    GLU_TRY(check_aligned(a_keys, kb, "a_keys", "the key size"));
    GLU_TRY(check_aligned(b_keys, kb, "b_keys", "the key size"));
    GLU_TRY(check_aligned(out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(a_vals, "a_vals"));
    GLU_TRY(check_aligned_4(b_vals, "b_vals"));
    GLU_TRY(check_aligned_4(out_vals, "out_vals"));
    GLU_TRY(check_disjoint({{out_keys, total * kb, "out_keys"}, {out_vals, total * 4, "out_vals"}},
                           {{a_keys, a_count * kb, "a_keys"}, {b_keys, b_count * kb, "b_keys"}, {a_vals, a_count * 4, "a_vals"}, {b_vals, b_count * 4, "b_vals"}},
                           kOutputsAfterInputs));

    const MergePlan p = merge_plan(total, kb, with_vals);
    merge->last = {p.tiles, p.kernels};
    if (!total) return GLU_OK;
    GLU_TRY(merge->split.reserve(p.scratch_bytes));
    const hipStream_t st = pick_stream(stream);
    return kb == 8 ? run<uint64_t>(merge, a_keys, a_vals, a_count, b_keys, b_vals, b_count, out_keys, out_vals, (int) key_type, p, st)
                   : run<uint32_t>(merge, a_keys, a_vals, a_count, b_keys, b_vals, b_count, out_keys, out_vals, (int) key_type, p, st);
}

glu_status glu_merge_plan_batch(size_t total_count, size_t num_segments, glu_key_type key_type, int with_vals, uint32_t* tile, uint32_t* tiles,
                                uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_total(total_count, 0));
    GLU_TRY(check_batch_segments(num_segments));
    const MergePlan p = merge_batch_plan(total_count, num_segments, key_bytes_of((int) key_type), with_vals != 0);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_merge_prepare_batch(glu_merge merge, size_t total_count, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_total(total_count, 0));
    // (the tile is the same with and without values; the boundaries do not depend on the number of segments)
    return merge->split.reserve(merge_batch_plan(total_count, 1, key_bytes_of((int) key_type), true).scratch_bytes);
}

glu_status glu_merge_run_batch_offsets_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, const uint32_t* a_offsets, size_t a_total,
                                           const void* b_keys, const uint32_t* b_vals, const uint32_t* b_offsets, size_t b_total,
                                           size_t num_segments, void* out_keys, uint32_t* out_vals, uint32_t* out_offsets, glu_key_type key_type,
                                           void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_batch_segments(num_segments));
    if (num_segments && (!a_offsets || !b_offsets)) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid %s array", a_offsets ? "b_offsets" : "a_offsets");
    GLU_TRY(check_aligned_4(a_offsets, "a_offsets"));
    GLU_TRY(check_aligned_4(b_offsets, "b_offsets"));
    if (!num_segments) a_offsets = b_offsets = nullptr; // (not looked at)
    return merge_batch(merge, {a_keys, b_keys, a_vals, b_vals, a_offsets, b_offsets, 0, 0, a_total, b_total, num_segments, out_keys, out_vals,
                               out_offsets, (int) key_type, stream});
}

glu_status glu_merge_run_batch_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, size_t a_len, const void* b_keys,
                                   const uint32_t* b_vals, size_t b_len, size_t num_segments, void* out_keys, uint32_t* out_vals,
                                   uint32_t* out_offsets, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_total(a_len, b_len)); // (each below 2^32: the products below do not wrap)
    return merge_batch(merge, {a_keys, b_keys, a_vals, b_vals, nullptr, nullptr, a_len, b_len, num_segments * a_len, num_segments * b_len,
                               num_segments, out_keys, out_vals, out_offsets, (int) key_type, stream});
}

glu_status glu_merge_last(glu_merge merge, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    store(tiles, merge->last.tiles);
    store(kernels, merge->last.kernels);
    return GLU_OK;
}


// ---- set operations

glu_status glu_set_ops_plan(size_t a_count, size_t b_count, glu_key_type key_type, int with_arrays, uint32_t* tile, uint32_t* tiles,
                            uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_set_total(a_count, b_count));
    const SetOpsPlan p = set_ops_plan((uint64_t) a_count + b_count, key_bytes_of((int) key_type), with_arrays != 0);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_set_ops_create(glu_set_ops* out) { return create_object(out); }

glu_status glu_set_ops_destroy(glu_set_ops set_ops) { return destroy_object(set_ops); }

glu_status glu_set_ops_prepare(glu_set_ops set_ops, size_t total_count, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_set_total(total_count, 0));
    return set_ops->scratch.reserve(set_ops_plan(total_count, key_bytes_of((int) key_type), true).scratch_bytes);
}

glu_status glu_set_ops_run_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals, size_t a_count, const void* b_keys,
                               const uint32_t* b_vals, size_t b_count, void* out_keys, uint32_t* out_vals, size_t max_out, uint32_t* num_out,
                               glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    if (op < 0 || op >= GLU_SET_OP_COUNT_)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "op must be one of GLU_SET_UNION .. GLU_SET_SYMMETRIC_DIFFERENCE (got %d)", op);
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_set_total(a_count, b_count));
    GLU_TRY(check_below_2_32(max_out, "max_out"));
    const uint32_t kb = key_bytes_of((int) key_type);
    const size_t total = a_count + b_count;
    // a side of no elements is not looked at
    if (!a_count) a_keys = nullptr, a_vals = nullptr;
    if (!b_count) b_keys = nullptr, b_vals = nullptr;
    if (a_count && !a_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid a_keys buffer");
    if (b_count && !b_keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid b_keys buffer");
    if (!num_out) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_out pointer");
    const bool with_arrays = out_keys != nullptr && max_out != 0; // (else the call only counts)
    if (out_vals && !with_arrays)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "out_vals needs out_keys and max_out > 0 (a call that only counts takes neither)");
    const bool with_vals = out_vals != nullptr;
    if (a_count && (a_vals != nullptr) != with_vals)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "a_vals and out_vals must both be given or both be NULL");
    // B's values are read exactly where its elements can be written
    const bool b_written = with_vals && set_op_keeps_b((uint32_t) op) && b_count;
    if (b_written && !b_vals) return fail(GLU_ERROR_INVALID_ARGUMENT, "b_vals is required: the operation can write elements of B");
    if (!b_written) b_vals = nullptr;
    GLU_TRY(check_aligned(a_keys, kb, "a_keys", "the key size"));
    GLU_TRY(check_aligned(b_keys, kb, "b_keys", "the key size"));
    GLU_TRY(check_aligned(out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(a_vals, "a_vals"));
    GLU_TRY(check_aligned_4(b_vals, "b_vals"));
    GLU_TRY(check_aligned_4(out_vals, "out_vals"));
    GLU_TRY(check_aligned_4(num_out, "num_out"));
    // (no more than min(bound, max_out) entries of an output array can be written)
    const size_t room = with_arrays ? (size_t) std::min<uint64_t>(set_op_bound((uint32_t) op, a_count, b_count), max_out) : 0;
    GLU_TRY(check_disjoint({{out_keys, room * kb, "out_keys"}, {out_vals, room * 4, "out_vals"}, {num_out, sizeof(uint32_t), "num_out"}},
                           {{a_keys, a_count * kb, "a_keys"}, {b_keys, b_count * kb, "b_keys"}, {a_vals, a_count * 4, "a_vals"}, {b_vals, b_count * 4, "b_vals"}},
                           kOutputsAfterInputs));

    const SetOpsPlan p = set_ops_plan(total, kb, with_arrays);
    GLU_TRY(set_ops->scratch.reserve(p.scratch_bytes));
    set_ops->last = {p.tiles, p.kernels};
    const SetCall c{set_ops, op, a_keys, b_keys, a_vals, b_vals, a_count, b_count, out_keys, out_vals, room, num_out, (int) key_type, pick_stream(stream)};
    return kb == 8 ? set_run<uint64_t>(c, p, with_arrays) : set_run<uint32_t>(c, p, with_arrays);
}

glu_status glu_set_ops_plan_batch(size_t a_total, size_t b_total, size_t num_segments, glu_key_type key_type, int with_arrays, int with_offsets,
                                  uint32_t* tile, uint32_t* tiles, uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_set_total(a_total, b_total));
    GLU_TRY(check_batch_segments(num_segments));
    const SetOpsPlan p = set_ops_batch_plan((uint64_t) a_total + b_total, num_segments, key_bytes_of((int) key_type), with_arrays != 0, with_offsets != 0);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_set_ops_prepare_batch(glu_set_ops set_ops, size_t total_count, size_t num_segments, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_set_total(total_count, 0));
    GLU_TRY(check_batch_segments(num_segments));
    // (the scratch follows from the tiles alone; a call with arrays and out_offsets takes the most)
    return set_ops->scratch.reserve(set_ops_batch_plan(total_count, num_segments, key_bytes_of((int) key_type), true, true).scratch_bytes);
}

glu_status glu_set_ops_run_batch_offsets_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals, const uint32_t* a_offsets,
                                             size_t a_total, const void* b_keys, const uint32_t* b_vals, const uint32_t* b_offsets, size_t b_total,
                                             size_t num_segments, void* out_keys, uint32_t* out_vals, size_t max_out, uint32_t* out_offsets,
                                             uint32_t* num_out, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_batch_segments(num_segments));
    if (num_segments && (!a_offsets || !b_offsets)) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid %s array", a_offsets ? "b_offsets" : "a_offsets");
    GLU_TRY(check_aligned_4(a_offsets, "a_offsets"));
    GLU_TRY(check_aligned_4(b_offsets, "b_offsets"));
    if (!num_segments) a_offsets = b_offsets = nullptr; // (not looked at)
    return set_ops_batch(set_ops, {op, a_keys, b_keys, a_vals, b_vals, a_offsets, b_offsets, 0, 0, a_total, b_total, num_segments, out_keys, out_vals,
                                   max_out, out_offsets, num_out, (int) key_type, stream});
}

glu_status glu_set_ops_run_batch_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals, size_t a_len, const void* b_keys,
                                     const uint32_t* b_vals, size_t b_len, size_t num_segments, void* out_keys, uint32_t* out_vals, size_t max_out,
                                     uint32_t* out_offsets, uint32_t* num_out, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_set_total(a_len, b_len)); // (each below 2^32: the products below do not wrap)
    return set_ops_batch(set_ops, {op, a_keys, b_keys, a_vals, b_vals, nullptr, nullptr, a_len, b_len, num_segments * a_len, num_segments * b_len,
                                   num_segments, out_keys, out_vals, max_out, out_offsets, num_out, (int) key_type, stream});
}

glu_status glu_set_ops_last(glu_set_ops set_ops, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(set_ops, "set_ops"));
    store(tiles, set_ops->last.tiles);
    store(kernels, set_ops->last.kernels);
    return GLU_OK;
}

} // extern "C"
