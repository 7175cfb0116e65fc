// glu_top_k.hip -- top-k of libglu_hip.so (topk_kernels.hpp over topk_pick.hpp): glu_top_k_create, glu_top_k_destroy,
// glu_top_k_prepare, glu_top_k_set_option, glu_top_k_run_ptr, glu_top_k_read_last, glu_top_k_plan.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "glu_top_k_object.hpp"
#include "topk_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(GLU_TOP_K_PATH_AUTO == TOPK_PATH_AUTO && GLU_TOP_K_PATH_CANDIDATES == TOPK_PATH_CANDIDATES && GLU_TOP_K_PATH_FULL == TOPK_PATH_FULL,
              "the header's paths are the kernels'");
static_assert(kKeyXfNone == KEY_XF_NONE && kKeyXfSigned == KEY_XF_SIGNED && kKeyXfFloat == KEY_XF_FLOAT, "glu_args.hpp states the key transforms");
static_assert(sizeof(TopkState) % 8 == 0, "the column sums behind the state are read as pairs of words");

namespace
{
constexpr size_t kMaxCapacity = (size_t) 1 << 30;

glu_status check_sizes(size_t count, size_t k, int key_type)
{
    GLU_TRY(check_key_type(key_type));
    GLU_TRY(check_tile_count(count, "top-k takes a count below 2^32"));
    if (k > count) return fail(GLU_ERROR_INVALID_ARGUMENT, "k must not exceed count (got k %zu, count %zu)", k, count);
    return GLU_OK;
}

// what prepare and a call reserve: everything but the pairs of the ordering and the sort behind them
glu_status reserve_select(glu_top_k_s* t, size_t count, uint32_t kb)
{
    if (!count) return GLU_OK;
    const TopkPlan p = topk_plan(count, 1, kb, false, false, t->path, t->capacity);
    GLU_TRY(t->state.reserve(sizeof(TopkState) + kTopkBins * sizeof(uint32_t)));
    GLU_TRY(t->partial.reserve((size_t) std::min(p.tiles + 1u, kTopkGroupsMax) * kTopkBins * sizeof(uint32_t))); // (one tile more: tile_span.hpp)
    GLU_TRY(t->cand.reserve((size_t) p.capacity * kb));
    GLU_TRY(t->less_counts.reserve(count, kb, kTopkPacks));
    return t->tie_counts.reserve(count, kb, kTopkPacks);
}

glu_status reserve_ordering(glu_top_k_s* t, size_t max_k, uint32_t kb)
{
    if (!max_k) return GLU_OK;
    if (!t->sort)
    {
        GLU_TRY(glu_radix_sort_create(&t->sort));
        GLU_TRY(glu_radix_sort_set_option(t->sort, "SCRATCH_TUNE", 0)); // (k pairs: no placement by measurement)
    }
    GLU_TRY(t->pairs.reserve(max_k * (kb + sizeof(uint32_t))));
    return glu_radix_sort_prepare_ex(t->sort, max_k, kb, 1);
}

struct Call
{
    glu_top_k_s* t;
    const void* keys;
    int key_type;
    size_t count, k;
    bool largest, sorted;
    void* out_keys;
    uint32_t* out_indices;
    void* out_kth;
    hipStream_t stream;
};

// The launch sequence follows from count, k, the key width, `sorted`, which outputs are given, the address of keys and the options.
template<typename K>
glu_status run(const Call& c)
{
    glu_top_k_s* t = c.t;
    const bool arrays = c.out_keys || c.out_indices;
    TopkArgs<K> a;
    a.keys = tile_span<K, kTopkPacks>(c.keys, c.count);
    a.code.xf = key_xf_of(c.key_type);
    a.code.largest = c.largest ? 1u : 0u;
    const uint32_t tiles = a.keys.tiles, groups = std::min(tiles, kTopkGroupsMax), grid = tile_grid(tiles);
    const uint32_t rounds = topk_rounds(sizeof(K)), k = (uint32_t) c.k, count = (uint32_t) c.count;
    const uint32_t capacity = t->capacity ? t->capacity : topk_default_capacity(c.count);
    TopkState* state = (TopkState*) t->state.ptr;
    uint32_t* sums = (uint32_t*) ((char*) t->state.ptr + sizeof(TopkState));
    uint32_t* partial = (uint32_t*) t->partial.ptr;
    K* out_kth = (K*) c.out_kth;
    uint32_t kernels = 0;
    const auto round_over_input = [&](uint32_t r) {
        hipLaunchKernelGGL((topk_count_kernel<K>), dim3(groups), dim3(kTopkThreads), 0, c.stream, a, r, (const TopkState*) state, partial);
        hipLaunchKernelGGL(topk_sum_kernel, dim3(kTopkBins / kTopkSumCols), dim3(kTopkSumThreads), 0, c.stream, (const uint32_t*) partial, groups, r,
                           (const TopkState*) state, sums);
        hipLaunchKernelGGL((topk_pick_kernel<K>), dim3(1), dim3(kTopkPickThreads), 0, c.stream, (const uint32_t*) sums, r, count, k, t->path,
                           capacity, a.code, state, out_kth);
        kernels += 3;
    };
    round_over_input(0);
    HIP_TRY(hipGetLastError());
    if (t->path != (uint32_t) TOPK_PATH_FULL)
    {
        hipLaunchKernelGGL((topk_collect_kernel<K>), dim3(grid), dim3(kTopkThreads), 0, c.stream, a, state, (K*) t->cand.ptr, capacity);
        hipLaunchKernelGGL((topk_cand_rounds_kernel<K>), dim3(1), dim3(kTopkPickThreads), 0, c.stream, (const K*) t->cand.ptr, capacity, a.code,
                           state, out_kth);
        kernels += 2;
        HIP_TRY(hipGetLastError());
    }
    for (uint32_t r = 1; r < rounds; r++) round_over_input(r);
    HIP_TRY(hipGetLastError());
    if (arrays)
    {
        uint32_t* less_counts = (uint32_t*) t->less_counts.ptr;
        uint32_t* tie_counts = (uint32_t*) t->tie_counts.ptr;
        hipLaunchKernelGGL((topk_flag_count_kernel<K>), dim3(grid), dim3(kTopkThreads), 0, c.stream, a, (const TopkState*) state, less_counts,
                           tie_counts);
        HIP_TRY(hipGetLastError());
        GLU_TRY(launch_tile_count_scan(less_counts, tiles, &state->totals[0], c.stream));
        GLU_TRY(launch_tile_count_scan(tie_counts, tiles, &state->totals[1], c.stream));
        K* pair_codes = (K*) t->pairs.ptr;
        uint32_t* pair_indices = (uint32_t*) ((char*) t->pairs.ptr + c.k * sizeof(K));
        if (c.sorted)
            hipLaunchKernelGGL((topk_write_kernel<K, true>), dim3(grid), dim3(kTopkThreads), 0, c.stream, a, (const TopkState*) state,
                               (const uint32_t*) less_counts, (const uint32_t*) tie_counts, k, pair_codes, pair_indices);
        else
            hipLaunchKernelGGL((topk_write_kernel<K, false>), dim3(grid), dim3(kTopkThreads), 0, c.stream, a, (const TopkState*) state,
                               (const uint32_t*) less_counts, (const uint32_t*) tie_counts, k, (K*) c.out_keys, c.out_indices);
        HIP_TRY(hipGetLastError());
        kernels += 4;
        if (c.sorted)
        {
            // unsigned, stable, ascending by the code word: best first, equal keys by ascending index (the pairs are in index order)
            if (sizeof(K) == 4) GLU_TRY(glu_radix_sort_run_ptr(t->sort, (uint32_t*) pair_codes, pair_indices, c.k, 0, c.stream));
            else GLU_TRY(glu_radix_sort_run_u64_ptr(t->sort, (uint64_t*) pair_codes, pair_indices, c.k, 0, c.stream));
            hipLaunchKernelGGL((topk_decode_kernel<K>), dim3((k + kTopkDecodeThreads - 1) / kTopkDecodeThreads), dim3(kTopkDecodeThreads), 0, c.stream,
                               (const K*) pair_codes, (const uint32_t*) pair_indices, k, a.code, (K*) c.out_keys, c.out_indices);
            HIP_TRY(hipGetLastError());
            kernels += 2;
        }
    }
    t->last_kernels = kernels;
    t->ran = true;
    return GLU_OK;
}
} // namespace

extern "C" {

glu_status glu_top_k_plan(size_t count, size_t k, glu_key_type key_type, int sorted, int with_arrays, int path, size_t cand_capacity,
                          uint32_t* rounds, uint32_t* digit_shift, uint32_t* digit_bits, uint32_t* tile, uint32_t* tiles, uint32_t* capacity,
                          uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_sizes(count, k, (int) key_type));
    if (path < GLU_TOP_K_PATH_AUTO || path > GLU_TOP_K_PATH_FULL)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "path must be GLU_TOP_K_PATH_AUTO, _CANDIDATES or _FULL (0 .. 2) (got %d)", path);
    if (cand_capacity > kMaxCapacity) return fail(GLU_ERROR_INVALID_ARGUMENT, "cand_capacity must be at most 2^30 (got %zu)", cand_capacity);
    const uint32_t kb = key_bytes_of((int) key_type);
    const TopkPlan p = topk_plan(count, k, kb, with_arrays != 0, sorted != 0, (uint32_t) path, (uint32_t) cand_capacity);
    store(rounds, p.rounds);
    for (uint32_t r = 0; r < p.rounds; r++)
    {
        if (digit_shift) digit_shift[r] = topk_shift(kb, r);
        if (digit_bits) digit_bits[r] = topk_bits(kb, r);
    }
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(capacity, p.capacity);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_top_k_create(glu_top_k* out) { return create_object(out); }

glu_status glu_top_k_destroy(glu_top_k top_k) { return destroy_object(top_k); }

glu_status glu_top_k_set_option(glu_top_k top_k, const char* name, long long value)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    GLU_TRY(check_not_null(name, "name"));
    if (!strcmp(name, "PATH"))
    {
        if (value < GLU_TOP_K_PATH_AUTO || value > GLU_TOP_K_PATH_FULL)
            return fail(GLU_ERROR_INVALID_ARGUMENT, "PATH must be GLU_TOP_K_PATH_AUTO, _CANDIDATES or _FULL (0 .. 2) (got %lld)", value);
        top_k->path = (uint32_t) value;
        return GLU_OK;
    }
    if (!strcmp(name, "CAND_CAPACITY"))
    {
        if (value < 0 || value > (long long) kMaxCapacity)
            return fail(GLU_ERROR_INVALID_ARGUMENT, "CAND_CAPACITY must lie in [0, 2^30], 0 being the default of the count (got %lld)", value);
        top_k->capacity = (uint32_t) value;
        return GLU_OK;
    }
    if (!strcmp(name, "BATCH_LOOP_MIN")) // (the batched calls, glu_top_k_batch.hip)
    {
        if (value < 0 || value >= (long long) 1 << 32)
            return fail(GLU_ERROR_INVALID_ARGUMENT, "BATCH_LOOP_MIN must lie in [0, 2^32), 0 being the default (got %lld)", value);
        top_k->batch_loop_min = (uint64_t) value;
        return GLU_OK;
    }
    return fail(GLU_ERROR_INVALID_ARGUMENT, "Unknown option: %s (the options are PATH, CAND_CAPACITY and BATCH_LOOP_MIN)", name);
}

glu_status glu_top_k_prepare(glu_top_k top_k, size_t count, size_t max_k, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    GLU_TRY(check_sizes(count, max_k, (int) key_type));
    const uint32_t kb = key_bytes_of((int) key_type);
    GLU_TRY(reserve_select(top_k, count, kb));
    return reserve_ordering(top_k, max_k, kb);
}

glu_status glu_top_k_run_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t count, size_t k, int largest, int sorted,
                             void* out_keys, uint32_t* out_indices, void* out_kth, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    GLU_TRY(check_sizes(count, k, (int) key_type));
    if (count && !keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid keys buffer");
    if (!out_keys && !out_indices && !out_kth) return fail(GLU_ERROR_INVALID_ARGUMENT, "out_keys, out_indices and out_kth are all NULL");
    const uint32_t kb = key_bytes_of((int) key_type);
    GLU_TRY(check_aligned(keys, kb, "keys", "the key size"));
    GLU_TRY(check_aligned(out_keys, kb, "out_keys", "the key size"));
    GLU_TRY(check_aligned_4(out_indices, "out_indices"));
    GLU_TRY(check_aligned(out_kth, kb, "out_kth", "the key size"));
    GLU_TRY(check_disjoint({{out_keys, k * kb, "out_keys"}, {out_indices, k * sizeof(uint32_t), "out_indices"}, {out_kth, k ? kb : 0, "out_kth"}},
                           {{keys, count * kb, "keys"}}, kOutputsAfterInputs));
    if (!k) // (nothing is written, out_kth neither)
    {
        top_k->last_kernels = 0;
        top_k->ran = false;
        return GLU_OK;
    }
    GLU_TRY(reserve_select(top_k, count, kb));
    if (sorted && (out_keys || out_indices)) GLU_TRY(reserve_ordering(top_k, k, kb));
    const Call c{top_k, keys, (int) key_type, count, k, largest != 0, sorted != 0, out_keys, out_indices, out_kth, pick_stream(stream)};
    return kb == 4 ? run<uint32_t>(c) : run<uint64_t>(c);
}

glu_status glu_top_k_read_last(glu_top_k top_k, uint32_t* path, uint32_t* candidates, uint32_t* ties, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(top_k, "top_k"));
    TopkState s = {};
    if (top_k->ran) HIP_TRY(hipMemcpy(&s, top_k->state.ptr, sizeof(s), hipMemcpyDeviceToHost));
    store(path, s.path);
    store(candidates, s.path == (uint32_t) TOPK_PATH_CANDIDATES ? s.cand : 0u);
    store(ties, s.need);
    store(kernels, top_k->last_kernels);
    return GLU_OK;
}

} // extern "C"
