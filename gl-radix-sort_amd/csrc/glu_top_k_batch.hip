// glu_top_k_batch.hip -- batched top-k of libglu_hip.so (topk_batch_kernels.hpp over topk_batch_plan.hpp): glu_top_k_run_batch_ptr,
// glu_top_k_run_batch_offsets_ptr, glu_top_k_prepare_batch, glu_top_k_plan_batch, glu_top_k_read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "glu_top_k_object.hpp"
#include "topk_batch_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(kKeyXfNone == KEY_XF_NONE && kKeyXfSigned == KEY_XF_SIGNED && kKeyXfFloat == KEY_XF_FLOAT, "glu_args.hpp states the key transforms");
static_assert(GLU_TOP_K_BATCH_NONE == TOPK_BATCH_NONE && GLU_TOP_K_BATCH_WAVE == TOPK_BATCH_WAVE && GLU_TOP_K_BATCH_BLOCK == TOPK_BATCH_BLOCK &&
                  GLU_TOP_K_BATCH_LONG == TOPK_BATCH_LONG && GLU_TOP_K_BATCH_LOOP == TOPK_BATCH_LOOP && GLU_TOP_K_BATCH_BINNED == TOPK_BATCH_BINNED,
              "the header's paths are the plan's");
static_assert(kBatchCountWords == 64, "topk_batch_plan.hpp counts the line of counts in its scratch bytes");

namespace
{
struct Sizes
{
    bool offsets_form;
    size_t count;        // equal partitions: keys per partition
    size_t total, num_segments, k;
    int key_type;
};

// what the host can check of the sizes of a batch, each refusal naming its argument
glu_status check_sizes(const Sizes& z)
{
    GLU_TRY(check_key_type(z.key_type));
    GLU_TRY(check_batch_segments(z.num_segments));
    if (!z.offsets_form)
    {
        if (z.count && z.num_segments > ((size_t) -1) / z.count) return fail(GLU_ERROR_INVALID_ARGUMENT, "count * num_partitions overflows");
        if (z.k > z.count) return fail(GLU_ERROR_INVALID_ARGUMENT, "k must not exceed count (got k %zu, count %zu)", z.k, z.count);
    }
    GLU_TRY(check_batch_total(z.offsets_form ? z.total : z.count * z.num_segments));
    if (z.k && z.num_segments > (((size_t) 1 << 32) - 1) / z.k)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments * k must stay below 2^32 (got num_segments %zu, k %zu)", z.num_segments, z.k);
    return GLU_OK;
}

// the ordering of rows of k pairs: beyond the batched sort's single-block limit it is one ordinary sort per row
bool rows_sorted_singly(size_t k, uint32_t kb)
{
    uint32_t path = 0, tile = 0;
    (void) glu_radix_sort_plan_batch(k, kb, 1, &path, &tile);
    return path == 3;
}

TopkBatchPlan plan_of(const glu_top_k_s* t, const Sizes& z, bool arrays, bool sorted)
{
    const uint32_t kb = key_bytes_of(z.key_type);
    const uint64_t loop_min = t ? t->batch_loop_min : 0;
    const size_t per_call = z.offsets_form ? 0 : z.count;
    const TopkPlan single = topk_plan(per_call, std::min(z.k, per_call), kb, arrays, sorted, t ? t->path : (uint32_t) TOPK_PATH_AUTO, t ? t->capacity : 0u);
    return topk_batch_plan(z.offsets_form, z.offsets_form ? z.total : z.count, z.num_segments, z.k, kb, arrays, sorted, loop_min,
                           rows_sorted_singly(z.k, kb), single);
}

template<typename K, int GEO>
struct BlockGeo
{
    static constexpr int THREADS = (int) topk_batch_tile_threads(GEO);
    static constexpr int TILE = (int) (topk_batch_tile_bytes(GEO) / sizeof(K));
    static constexpr size_t LDS = topk_batch_block_lds<K, THREADS, TILE>();
};

// the LDS opt-in of a workgroup class's kernel, once
template<typename K, int GEO>
glu_status block_kernel_opt_in()
{
    using G = BlockGeo<K, GEO>;
    static std::once_flag once;
    static hipError_t result = hipSuccess;
    std::call_once(once, [&] {
        result = hipFuncSetAttribute((const void*) topk_batch_block_kernel<K, G::THREADS, G::TILE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int) G::LDS);
    });
    HIP_TRY(result);
    return GLU_OK;
}

template<typename K>
glu_status block_opt_in_all()
{
    GLU_TRY((block_kernel_opt_in<K, 0>()));
    GLU_TRY((block_kernel_opt_in<K, 1>()));
    return block_kernel_opt_in<K, 2>();
}

template<typename K, int GEO>
glu_status launch_block_geo(const TopkBatchArgs<K>& a, uint32_t capacity, uint32_t per_cu, hipStream_t stream)
{
    using G = BlockGeo<K, GEO>;
    GLU_TRY((block_kernel_opt_in<K, GEO>()));
    const uint32_t grid = std::min<uint32_t>(capacity, cus() * per_cu);
    hipLaunchKernelGGL((topk_batch_block_kernel<K, G::THREADS, G::TILE>), dim3(grid), dim3(G::THREADS), G::LDS, stream, a);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// the kernel of list c over `capacity` entries at the most (workgroups that share a CU by LDS and waves: 8 / 2 / 1 of the tiles)
template<typename K>
glu_status launch_class(const TopkBatchArgs<K>& a, int c, uint32_t capacity, hipStream_t stream)
{
    if (!capacity) return GLU_OK;
    if (c == 0)
    {
        const uint32_t grid = std::min<uint32_t>((capacity + kTopkBatchWaveWaves - 1) / kTopkBatchWaveWaves, cus() * 8u);
        hipLaunchKernelGGL((topk_batch_wave_kernel<K>), dim3(grid), dim3(kTopkBatchWaveWaves * 64u), 0, stream, a);
    }
    else if (c == 1) return launch_block_geo<K, 0>(a, capacity, 8, stream);
    else if (c == 2) return launch_block_geo<K, 1>(a, capacity, 2, stream);
    else if (c == 3) return launch_block_geo<K, 2>(a, capacity, 1, stream);
    else
        hipLaunchKernelGGL((topk_batch_long_kernel<K>), dim3(std::min<uint32_t>(capacity, cus() * 2u)), dim3(kTopkBatchLongThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

glu_status reserve_rows(glu_top_k_s* t, size_t num_segments, size_t k, uint32_t kb)
{
    if (!t->sort)
    {
        GLU_TRY(glu_radix_sort_create(&t->sort));
        GLU_TRY(glu_radix_sort_set_option(t->sort, "SCRATCH_TUNE", 0)); // (rows of k pairs: no placement by measurement)
    }
    GLU_TRY(t->batch_rows.reserve(num_segments * k * (kb + sizeof(uint32_t))));
    return glu_radix_sort_prepare_batch(t->sort, num_segments * k, num_segments, kb, 1);
}

struct Call
{
    glu_top_k_s* t;
    Sizes z;
    const void* keys;
    const uint32_t* offsets;
    bool largest, sorted;
    void* out_keys;
    uint32_t* out_indices;
    void* out_kth;
    hipStream_t stream;
};

// The launch sequence follows from the sizes, `sorted`, which outputs are given and the options.
template<typename K>
glu_status run(const Call& c, const TopkBatchPlan& plan)
{
    glu_top_k_s* t = c.t;
    const Sizes& z = c.z;
    const uint32_t kb = sizeof(K);
    const bool arrays = c.out_keys || c.out_indices, pairs = arrays && c.sorted;
    const size_t entries = z.num_segments * z.k;
    TopkBatchArgs<K> a = {};
    a.keys = (const K*) c.keys;
    a.offsets = c.offsets;
    a.count = (uint32_t) z.count;
    a.total = (uint32_t) z.total;
    a.nsegs = (uint32_t) z.num_segments;
    a.code.xf = key_xf_of(z.key_type);
    a.code.largest = c.largest ? 1u : 0u;
    a.k = (uint32_t) z.k;
    a.pairs = pairs ? 1u : 0u;
    a.out_keys = (K*) c.out_keys;
    a.out_indices = c.out_indices;
    a.out_kth = (K*) c.out_kth;
    K* pair_codes = nullptr;
    uint32_t* pair_indices = nullptr;
    if (pairs)
    {
        GLU_TRY(reserve_rows(t, z.num_segments, z.k, kb));
        pair_codes = (K*) t->batch_rows.ptr;
        pair_indices = (uint32_t*) ((char*) t->batch_rows.ptr + entries * kb);
        a.out_keys = pair_codes;
        a.out_indices = pair_indices;
    }
    if (z.offsets_form)
    {
        BatchListsLayout layout;
        uint32_t *counts, *lists, bin_grid;
        GLU_TRY(begin_batch_offsets(t->batch_lists, topk_batch_classes(kb), z.total, z.num_segments, c.stream, layout, counts, lists, bin_grid));
        hipLaunchKernelGGL(topk_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, c.stream, c.offsets, (uint32_t) z.num_segments, (uint32_t) z.total,
                           layout, counts, lists);
        HIP_TRY(hipGetLastError());
        for (int cls = 0; cls <= BATCH_LIST_LONG; cls++)
        {
            TopkBatchArgs<K> b = a;
            b.list = lists + layout.start[cls];
            b.list_count = counts + batch_count_word(cls);
            b.nsegs = layout.capacity[cls];
            GLU_TRY(launch_class(b, cls, layout.capacity[cls], c.stream));
        }
        t->last_batch.on_device = true;
    }
    else
    {
        GLU_TRY(launch_class(a, plan.list, (uint32_t) z.num_segments, c.stream));
        t->last_batch.by_class[plan.path - TOPK_BATCH_WAVE] = (uint32_t) z.num_segments;
    }
    if (pairs)
    {
        // unsigned, stable, ascending by the code word: best first, equal keys by ascending index (the rows are in index order), pads last
        GLU_TRY(glu_radix_sort_run_batch_ptr(t->sort, pair_codes, pair_indices, z.k, z.num_segments, kb == 4 ? GLU_KEY_UINT32 : GLU_KEY_UINT64,
                                             c.stream));
        const uint32_t grid = (uint32_t) std::min<size_t>((entries + kTopkBatchDecodeThreads - 1) / kTopkBatchDecodeThreads, (size_t) cus() * 64u);
        hipLaunchKernelGGL((topk_batch_decode_kernel<K>), dim3(grid), dim3(kTopkBatchDecodeThreads), 0, c.stream, (const K*) pair_codes,
                           (const uint32_t*) pair_indices, a, (K*) c.out_keys, c.out_indices);
        HIP_TRY(hipGetLastError());
    }
    return GLU_OK;
}

// what both entry points do behind their own checks
glu_status run_checked(const Call& c)
{
    glu_top_k_s* t = c.t;
    const Sizes& z = c.z;
    const uint32_t kb = key_bytes_of(z.key_type);
    const size_t total = z.offsets_form ? z.total : z.count * z.num_segments, entries = z.num_segments * z.k;
    if (total && !c.keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid keys buffer");
    if (!c.out_keys && !c.out_indices && !c.out_kth) return fail(GLU_ERROR_INVALID_ARGUMENT, "out_keys, out_indices and out_kth are all NULL");
    GLU_TRY(check_aligned(c.keys, kb, "keys", "the key size"));
    GLU_TRY(check_aligned(c.out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(c.out_indices, "out_indices"));
    GLU_TRY(check_aligned(c.out_kth, kb, "out_kth", "the key size"));
    GLU_TRY(check_disjoint({{c.out_keys, entries * kb, "out_keys"}, {c.out_indices, entries * sizeof(uint32_t), "out_indices"},
                            {c.out_kth, z.k ? z.num_segments * kb : 0, "out_kth"}},
                           {{c.keys, total * kb, "keys"}, {c.offsets, c.offsets ? (z.num_segments + 1) * sizeof(uint32_t) : 0, "the offsets array"}},
                           kOutputsAfterInputs));
    const bool arrays = c.out_keys || c.out_indices;
    const TopkBatchPlan plan = plan_of(t, z, arrays, c.sorted);
    t->last_batch.reset();
    t->last_batch_kernels = plan.kernels;
    if (plan.path == (uint32_t) TOPK_BATCH_NONE) return GLU_OK; // (nothing is written)
    if (plan.path == (uint32_t) TOPK_BATCH_LOOP)
    {
        // every partition fills the device by itself: the single call's chain, partition after partition, all on the caller's queue
        t->last_batch.by_class[2] = (uint32_t) z.num_segments;
        for (size_t p = 0; p < z.num_segments; p++)
            GLU_TRY(glu_top_k_run_ptr(t, (const char*) c.keys + p * z.count * kb, (glu_key_type) z.key_type, z.count, z.k, c.largest, c.sorted,
                                      c.out_keys ? (char*) c.out_keys + p * z.k * kb : nullptr, c.out_indices ? c.out_indices + p * z.k : nullptr,
                                      c.out_kth ? (char*) c.out_kth + p * kb : nullptr, c.stream));
        return GLU_OK;
    }
    return kb == 4 ? run<uint32_t>(c, plan) : run<uint64_t>(c, plan);
}
} // namespace

extern "C" {

glu_status glu_top_k_plan_batch(size_t count, size_t num_segments, size_t k, glu_key_type key_type, int offsets_form, int sorted, int with_arrays,
                                size_t loop_min, uint32_t* path, uint32_t* tile, uint32_t* class_limits, uint32_t* wave_digit_bits,
                                uint32_t* cand_room, size_t* loop_min_used, uint32_t* kernels, size_t* scratch_bytes)
{
    const Sizes z{offsets_form != 0, offsets_form ? 0 : count, offsets_form ? count : 0, num_segments, k, (int) key_type};
    GLU_TRY(check_sizes(z));
    if (loop_min >> 32) return fail(GLU_ERROR_INVALID_ARGUMENT, "loop_min must lie in [0, 2^32), 0 being the default (got %zu)", loop_min);
    const uint32_t kb = key_bytes_of((int) key_type);
    glu_top_k_s options; // (the defaults; only loop_min is the caller's)
    options.batch_loop_min = loop_min;
    const TopkBatchPlan p = plan_of(&options, z, with_arrays != 0, sorted != 0);
    store(path, p.path);
    store(tile, p.tile);
    if (class_limits)
        for (int c = 0; c < BATCH_LIST_LONG; c++) class_limits[c] = topk_batch_limit(c, kb);
    store(wave_digit_bits, kTopkBatchWaveDigitBits);
    store(cand_room, topk_batch_cand_room(kb));
    store(loop_min_used, (size_t) (loop_min ? loop_min : kTopkBatchLoopMinDefault));
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_top_k_prepare_batch(glu_top_k top_k, size_t total, size_t num_segments, size_t max_k, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    const Sizes z{true, 0, total, num_segments, max_k, (int) key_type};
    GLU_TRY(check_sizes(z));
    const uint32_t kb = key_bytes_of((int) key_type);
    BatchListsLayout layout;
    GLU_TRY(reserve_batch_lists(top_k->batch_lists, topk_batch_classes(kb), total, num_segments, layout));
    if (num_segments && max_k) GLU_TRY(reserve_rows(top_k, num_segments, max_k, kb));
    // equal partitions of this batch that go through the single call, partition after partition
    const uint64_t loop_min = top_k->batch_loop_min ? top_k->batch_loop_min : kTopkBatchLoopMinDefault;
    if (num_segments && total / num_segments >= loop_min)
        GLU_TRY(glu_top_k_prepare(top_k, total / num_segments, std::min(max_k, total / num_segments), key_type));
    // the LDS opt-in of the workgroup class's kernels, so that a first call under stream capture finds it made
    return kb == 4 ? block_opt_in_all<uint32_t>() : block_opt_in_all<uint64_t>();
}

glu_status glu_top_k_run_batch_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t count, size_t num_partitions, size_t k,
                                   int largest, int sorted, void* out_keys, uint32_t* out_indices, void* out_kth, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    const Sizes z{false, count, count * num_partitions, num_partitions, k, (int) key_type};
    GLU_TRY(check_sizes(z));
    return run_checked({top_k, z, keys, nullptr, largest != 0, sorted != 0, out_keys, out_indices, out_kth, pick_stream(stream)});
}

glu_status glu_top_k_run_batch_offsets_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t total, const uint32_t* offsets,
                                           size_t num_segments, size_t k, int largest, int sorted, void* out_keys, uint32_t* out_indices,
                                           void* out_kth, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    const Sizes z{true, 0, total, num_segments, k, (int) key_type};
    GLU_TRY(check_sizes(z));
    GLU_TRY(check_batch_offsets(offsets, num_segments));
    return run_checked({top_k, z, keys, num_segments ? offsets : nullptr, largest != 0, sorted != 0, out_keys, out_indices, out_kth,
                        pick_stream(stream)});
}

glu_status glu_top_k_read_batch(glu_top_k top_k, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    store(kernels, top_k->last_batch_kernels);
    return top_k->last_batch.read(top_k->batch_lists, 1, wave_segments, block_segments, long_segments); // (list 0: the wave class)
}

} // extern "C"
