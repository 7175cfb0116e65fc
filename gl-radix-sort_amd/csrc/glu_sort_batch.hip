// glu_sort_batch.hip -- the batched radix sort of libglu_hip.so (radix_batch_kernels.hpp): glu_radix_sort_run_batch_ptr,
// glu_radix_sort_run_batch_offsets_ptr, glu_radix_sort_prepare_batch, glu_radix_sort_plan_batch, glu_radix_sort_read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "glu_batch_host.hpp"
#include "glu_sort_driver.hpp"
#include "radix_batch_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// The tiles of the workgroup class (elements): 256 x 4, 1024 x 4 and the single-block limit (1024 x 16; 8-byte keys: 1024 x 8).
constexpr uint32_t batch_block_tile(int geo, size_t key_bytes)
{
    return geo == 0 ? 1024u : geo == 1 ? 4096u : key_bytes == 4 ? 16384u : 8192u;
}

// host only: path and tile of an equal-length batch (glu_radix_sort_plan_batch)
void plan_equal(size_t count, size_t key_bytes, uint32_t& path, uint32_t& tile, int& geo)
{
    geo = -1;
    if (count <= 1) { path = 0; tile = 0; return; }
    if (count <= kBatchWaveTile) { path = 1; tile = kBatchWaveTile; return; }
    for (int g = 0; g < 3; g++)
        if (count <= batch_block_tile(g, key_bytes)) { path = 2; tile = batch_block_tile(g, key_bytes); geo = g; return; }
    path = 3;
    tile = batch_block_tile(2, key_bytes);
}

// the classes of a batch with device offsets: segments of 2 elements and more; the wave class, the three tiles, longer ones
BatchClasses classes_of(size_t key_bytes)
{
    return {2, {kBatchWaveTile, batch_block_tile(0, key_bytes), batch_block_tile(1, key_bytes), batch_block_tile(2, key_bytes)}, 0, false};
}

template<typename KeyT, int THREADS, int KPT, bool VALS>
glu_status block_kernel_opt_in()
{
    using Smem = BatchBlockSmem<KeyT, THREADS, KPT, VALS>;
    static std::once_flag lds_opt_in;
    static hipError_t lds_opt_in_result = hipSuccess;
    std::call_once(lds_opt_in, [&] {
        lds_opt_in_result = hipFuncSetAttribute((const void*) radix_batch_block_kernel<KeyT, THREADS, KPT, VALS>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof(Smem));
    });
    HIP_TRY(lds_opt_in_result);
    return GLU_OK;
}

struct BatchArgs
{
    const uint32_t* offsets = nullptr; // device, or NULL: equal partitions of `count`
    uint32_t count = 0, total = 0, xf = 0;
    const uint32_t* lists = nullptr;   // device lists of a batch with device offsets (NULL: the segments themselves)
    const uint32_t* counts = nullptr;
    BatchListsLayout layout = {};
    uint32_t nsegs = 0;                // equal partitions: their number
};

// entries the kernel of list c walks at most, and where the list and its count lie
inline void list_of(const BatchArgs& a, int c, const uint32_t*& list, const uint32_t*& list_count, uint32_t& capacity)
{
    list = a.lists ? a.lists + a.layout.start[c] : nullptr;
    list_count = a.lists ? a.counts + batch_count_word(c) : nullptr;
    capacity = a.lists ? a.layout.capacity[c] : a.nsegs;
}

template<typename KeyT, bool VALS>
glu_status launch_wave(KeyT* keys, uint32_t* vals, const BatchArgs& a, hipStream_t stream)
{
    const uint32_t *list, *list_count;
    uint32_t capacity;
    list_of(a, 0, list, list_count, capacity);
    if (!capacity) return GLU_OK;
    const uint32_t grid = std::min<uint32_t>((capacity + kBatchWaveWaves - 1) / kBatchWaveWaves, (uint32_t) g_dev.num_cus * 8u);
    hipLaunchKernelGGL((radix_batch_wave_kernel<KeyT, VALS>), dim3(grid), dim3(kBatchWaveWaves * kWave), 0, stream, keys, vals, a.offsets,
                       a.count, a.total, list, list_count, capacity, a.xf);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

template<typename KeyT, int THREADS, int KPT, bool VALS>
glu_status launch_block_geo(KeyT* keys, uint32_t* vals, const BatchArgs& a, int c, uint32_t per_cu, hipStream_t stream)
{
    const uint32_t *list, *list_count;
    uint32_t capacity;
    list_of(a, c, list, list_count, capacity);
    if (!capacity) return GLU_OK;
    GLU_TRY((block_kernel_opt_in<KeyT, THREADS, KPT, VALS>()));
    const uint32_t grid = std::min<uint32_t>(capacity, (uint32_t) g_dev.num_cus * per_cu);
    hipLaunchKernelGGL((radix_batch_block_kernel<KeyT, THREADS, KPT, VALS>), dim3(grid), dim3(THREADS),
                       sizeof(BatchBlockSmem<KeyT, THREADS, KPT, VALS>), stream, keys, vals, a.offsets, a.count, a.total, list, list_count,
                       capacity, a.xf);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// tile geometry `geo` of the workgroup class (batch_block_tile): workgroups that share a CU by LDS and waves: 8 / 2 / 1
template<typename KeyT, bool VALS>
glu_status launch_block(KeyT* keys, uint32_t* vals, const BatchArgs& a, int geo, hipStream_t stream)
{
    constexpr int LARGE_KPT = sizeof(KeyT) == 4 ? 16 : 8;
    if (geo == 0) return launch_block_geo<KeyT, 256, 4, VALS>(keys, vals, a, 1, 8, stream);
    if (geo == 1) return launch_block_geo<KeyT, 1024, 4, VALS>(keys, vals, a, 2, 2, stream);
    return launch_block_geo<KeyT, 1024, LARGE_KPT, VALS>(keys, vals, a, 3, 1, stream);
}

template<typename KeyT, bool VALS>
glu_status block_opt_in_all()
{
    constexpr int LARGE_KPT = sizeof(KeyT) == 4 ? 16 : 8;
    GLU_TRY((block_kernel_opt_in<KeyT, 256, 4, VALS>()));
    GLU_TRY((block_kernel_opt_in<KeyT, 1024, 4, VALS>()));
    return block_kernel_opt_in<KeyT, 1024, LARGE_KPT, VALS>();
}

template<typename KeyT, bool VALS>
glu_status launch_long(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, const BatchArgs& a, hipStream_t stream)
{
    const uint32_t *list, *list_count;
    uint32_t capacity;
    list_of(a, BATCH_LIST_LONG, list, list_count, capacity);
    if (!capacity) return GLU_OK;
    const uint32_t grid = std::min<uint32_t>(capacity, (uint32_t) g_dev.num_cus);
    hipLaunchKernelGGL((radix_batch_long_kernel<KeyT, VALS>), dim3(grid), dim3(1024), 0, stream, keys, vals, (KeyT*) s->keys.ptr,
                       (uint32_t*) s->vals.ptr, a.offsets, a.total, list, list_count, capacity, a.xf);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

// device offsets: binning, then one kernel per list; seven launches whatever the segments look like
template<typename KeyT, bool VALS>
glu_status run_offsets(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t total, const uint32_t* offsets, size_t num_segments,
                       uint32_t xf, hipStream_t stream)
{
    // the long class sorts between the caller's arrays and the object's scratch arrays
    GLU_TRY(sort_prepare(s, total, sizeof(KeyT), VALS, false));
    BatchArgs a;
    a.offsets = offsets;
    a.total = (uint32_t) total;
    a.xf = xf;
    uint32_t *counts, *lists, bin_grid;
    GLU_TRY(begin_batch_offsets(s->batch_lists, classes_of(sizeof(KeyT)), total, num_segments, stream, a.layout, counts, lists, bin_grid));
    a.counts = counts;
    a.lists = lists;
    hipLaunchKernelGGL(radix_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, stream, offsets, (uint32_t) num_segments, (uint32_t) total,
                       a.layout, counts, lists);
    HIP_TRY(hipGetLastError());
    GLU_TRY((launch_wave<KeyT, VALS>(keys, vals, a, stream)));
    for (int geo = 0; geo < 3; geo++) GLU_TRY((launch_block<KeyT, VALS>(keys, vals, a, geo, stream)));
    GLU_TRY((launch_long<KeyT, VALS>(s, keys, vals, a, stream)));
    s->last_batch.on_device = true;
    return GLU_OK;
}

// equal partitions that fit a tile: the class is the host's decision, one launch
template<typename KeyT, bool VALS>
glu_status run_equal(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t count, size_t num_partitions, uint32_t path, int geo, uint32_t xf,
                     hipStream_t stream)
{
    BatchArgs a;
    a.count = (uint32_t) count;
    a.total = (uint32_t) (count * num_partitions);
    a.nsegs = (uint32_t) num_partitions;
    a.xf = xf;
    if (path == 1) return launch_wave<KeyT, VALS>(keys, vals, a, stream);
    return launch_block<KeyT, VALS>(keys, vals, a, geo, stream);
}

static_assert(kKeyXfNone == KEY_XF_NONE && kKeyXfSigned == KEY_XF_SIGNED && kKeyXfFloat == KEY_XF_FLOAT, "key_xf_of() speaks the kernels' KEY_XF_*");

glu_status check_arrays(const void* keys, const uint32_t* vals, size_t elements, glu_key_type key_type)
{
    GLU_TRY(check_key_type(key_type));
    GLU_TRY(check_batch_total(elements));
    if (elements && !keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid key buffer");
    GLU_TRY(check_aligned(keys, key_bytes_of(key_type), "the key array", "its element size"));
    return check_aligned(vals, sizeof(uint32_t), "the value array", "its element size");
}
} // namespace

extern "C" {

glu_status glu_radix_sort_plan_batch(size_t count, uint32_t key_bytes, int with_vals, uint32_t* path, uint32_t* tile)
{
    (void) with_vals; // (the tiles are those of pairs: keys-only batches take the same ones)
    if (key_bytes != 4 && key_bytes != 8) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bytes must be 4 or 8 (got %u)", key_bytes);
    uint32_t p, t;
    int geo;
    plan_equal(count, key_bytes, p, t, geo);
    store(path, p);
    store(tile, t);
    return GLU_OK;
}

glu_status glu_radix_sort_prepare_batch(glu_radix_sort sort, size_t total, size_t num_segments, size_t key_bytes, int with_vals)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (key_bytes != 4 && key_bytes != 8) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bytes must be 4 or 8 (got %zu)", key_bytes);
    GLU_TRY(check_batch_total(total));
    GLU_TRY(check_batch_segments(num_segments));
    BatchListsLayout layout;
    GLU_TRY(reserve_batch_lists(sort->batch_lists, classes_of(key_bytes), total, num_segments, layout));
    GLU_TRY(glu_radix_sort_prepare_ex(sort, total, key_bytes, with_vals)); // (the scratch arrays of the long class)
    // the LDS opt-in of the workgroup class's kernels, so that a first call under stream capture finds it made
    if (key_bytes == 4) return with_vals ? block_opt_in_all<uint32_t, true>() : block_opt_in_all<uint32_t, false>();
    return with_vals ? block_opt_in_all<uint64_t, true>() : block_opt_in_all<uint64_t, false>();
}

glu_status glu_radix_sort_run_batch_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count, size_t num_partitions,
                                        glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (count && num_partitions > ((size_t) -1) / count) return fail(GLU_ERROR_INVALID_ARGUMENT, "count * num_partitions overflows");
    GLU_TRY(check_arrays(keys, vals, count * num_partitions, key_type));
    GLU_TRY(check_batch_segments(num_partitions));
    const size_t key_bytes = key_bytes_of(key_type);
    uint32_t path, tile;
    int geo;
    plan_equal(count, key_bytes, path, tile, geo);
    sort->last_batch.reset();
    if (path == 0 || num_partitions == 0) return GLU_OK;
    sort->last_batch.by_class[path - 1] = (uint32_t) num_partitions;
    hipStream_t st = pick_stream(stream);
    if (path == 3)
    {
        // every partition is longer than an LDS tile: the ordinary sort, partition after partition, all on the caller's queue
        glu_status status = GLU_OK;
        for (size_t p = 0; p < num_partitions && status == GLU_OK; p++)
            status = sort_typed_one_queue(sort, (char*) keys + p * count * key_bytes, vals ? vals + p * count : nullptr, count, key_type, st);
        return status;
    }
    const uint32_t xf = key_xf_of(key_type);
    if (key_bytes == 4)
        return vals ? run_equal<uint32_t, true>(sort, (uint32_t*) keys, vals, count, num_partitions, path, geo, xf, st)
                    : run_equal<uint32_t, false>(sort, (uint32_t*) keys, nullptr, count, num_partitions, path, geo, xf, st);
    return vals ? run_equal<uint64_t, true>(sort, (uint64_t*) keys, vals, count, num_partitions, path, geo, xf, st)
                : run_equal<uint64_t, false>(sort, (uint64_t*) keys, nullptr, count, num_partitions, path, geo, xf, st);
}

glu_status glu_radix_sort_run_batch_offsets_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t total, const uint32_t* offsets,
                                                size_t num_segments, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    GLU_TRY(check_arrays(keys, vals, total, key_type));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_offsets(offsets, num_segments));
    sort->last_batch.reset();
    if (num_segments == 0 || total < 2) return GLU_OK; // (no segment can hold two elements)
    hipStream_t st = pick_stream(stream);
    const uint32_t xf = key_xf_of(key_type);
    if (key_bytes_of(key_type) == 4)
        return vals ? run_offsets<uint32_t, true>(sort, (uint32_t*) keys, vals, total, offsets, num_segments, xf, st)
                    : run_offsets<uint32_t, false>(sort, (uint32_t*) keys, nullptr, total, offsets, num_segments, xf, st);
    return vals ? run_offsets<uint64_t, true>(sort, (uint64_t*) keys, vals, total, offsets, num_segments, xf, st)
                : run_offsets<uint64_t, false>(sort, (uint64_t*) keys, nullptr, total, offsets, num_segments, xf, st);
}

glu_status glu_radix_sort_read_batch(glu_radix_sort sort, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    return sort->last_batch.read(sort->batch_lists, 1, wave_segments, block_segments, long_segments); // (list 0: the wave class)
}

} // extern "C"
