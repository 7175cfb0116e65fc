// glu_merge.hip -- merge of libglu_hip.so (merge_kernels.hpp): glu_merge_create, glu_merge_destroy, glu_merge_prepare,
// glu_merge_run_ptr, glu_merge_plan, glu_merge_last.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include "glu_merge_object.hpp"
#include "merge_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

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

glu_status glu_merge_last(glu_merge merge, uint32_t* tiles, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(merge, "merge"));
    store(tiles, merge->last.tiles);
    store(kernels, merge->last.kernels);
    return GLU_OK;
}

} // extern "C"
