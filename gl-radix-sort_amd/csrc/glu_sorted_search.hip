// glu_sorted_search.hip -- sorted search of libglu_hip.so (sorted_search_kernels.hpp): glu_sorted_search_create,
// glu_sorted_search_destroy, glu_sorted_search_prepare, glu_sorted_search_set_option, glu_sorted_search_index_ptr,
// glu_sorted_search_run_ptr, glu_sorted_search_plan, glu_sorted_search_last, and the batched search
// (sorted_search_batch_kernels.hpp over search_batch_walk.hpp): glu_sorted_search_run_batch_ptr,
// glu_sorted_search_run_batch_offsets_ptr, glu_sorted_search_set_batch_window, glu_sorted_search_plan_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "glu_sorted_search_object.hpp"
#include "sorted_search_batch_kernels.hpp"
#include "sorted_search_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(kSearchLevelsMax == kSearchMaxLevels, "the host's level rule fills the kernels' level table");
static_assert(kSearchBatchWindowUnset == GLU_SEARCH_BATCH_WINDOW_DEFAULT, "the header's default window is the walk's unset window");

namespace
{
glu_status check_hay_count(size_t n) { return check_tile_count(n, "sorted search takes a hay_count below 2^32"); }
glu_status check_needle_count(size_t n) { return check_tile_count(n, "sorted search takes a needle_count below 2^32"); }

uint32_t top_entries_of(uint32_t asked, uint32_t key_bytes) { return asked ? asked : search_lds_entries(key_bytes); }
glu_status check_top_entries(long long value, uint32_t key_bytes)
{
    // (0: the default.  One value serves both key widths only inside [32, 4096]; the call checks it against its own width.)
    if (value == 0 || (value >= (long long) search_fanout(key_bytes) && value <= (long long) search_lds_entries(key_bytes))) return GLU_OK;
    return fail(GLU_ERROR_INVALID_ARGUMENT, "TOP_ENTRIES must lie in [%u, %u] for %u-byte keys (got %lld)", search_fanout(key_bytes),
                search_lds_entries(key_bytes), key_bytes, value);
}

// DIRECT or INDEXED for a call that does not reuse an index: from the counts and the option, never from the data
int pick_path(int option, const SearchPlan& p, size_t hay_count, size_t needle_count)
{
    if (p.levels == 0 || option == GLU_SEARCH_PATH_DIRECT) return GLU_SEARCH_PATH_DIRECT;
    if (option == GLU_SEARCH_PATH_INDEXED) return GLU_SEARCH_PATH_INDEXED;
    return needle_count * kIndexNeedleRatio >= hay_count ? GLU_SEARCH_PATH_INDEXED : GLU_SEARCH_PATH_DIRECT;
}

// room for the index of `p`; an index that moved is no longer the index of anything
glu_status reserve_index(glu_sorted_search_s* s, const SearchPlan& p)
{
    const void* before = s->index.ptr;
    GLU_TRY(s->index.reserve(p.index_bytes));
    if (s->index.ptr != before) s->built.valid = false;
    return GLU_OK;
}

// one kernel: every level of the index written from the haystack
template<typename K>
glu_status launch_index(glu_sorted_search_s* s, const SearchPlan& p, const void* hay, int key_type, hipStream_t stream)
{
    SearchIndexArgs<K> a = {};
    a.hay = (const K*) hay;
    for (uint32_t k = 1; k <= p.levels; k++)
    {
        a.level[k] = (K*) ((char*) s->index.ptr + p.offset[k]);
        a.len[k] = p.len[k];
    }
    a.levels = p.levels;
    a.xf = key_xf_of(key_type);
    a.entries = p.entries;
    hipLaunchKernelGGL((sorted_search_index_kernel<K>), dim3((p.entries + kTileThreads - 1) / kTileThreads), dim3(kTileThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

struct Call
{
    glu_sorted_search_s* s;
    const void* hay;
    size_t hay_count;
    const void* needles;
    size_t needle_count;
    int key_type;
    uint32_t* out_lower;
    uint32_t* out_upper;
    hipStream_t stream;
};

template<typename K, int BOUNDS>
glu_status launch_search(const Call& c, const SearchPlan& p, bool indexed)
{
    if (!indexed)
    {
        // a lane slot per needle, up to 32 workgroups a CU (and then a loop)
        const uint32_t grid = std::max(1u, std::min((uint32_t) ((c.needle_count + kTileThreads - 1) / kTileThreads), cus() * 32u));
        hipLaunchKernelGGL((sorted_search_direct_kernel<K, BOUNDS>), dim3(grid), dim3(kTileThreads), 0, c.stream, (const K*) c.hay,
                           (uint32_t) c.hay_count, key_xf_of(c.key_type), (const K*) c.needles, (uint32_t) c.needle_count, c.out_lower,
                           c.out_upper);
    }
    else
    {
        const TileSpan<K> needles = tile_span<K, kSearchPacks>(c.needles, c.needle_count);
        const uint32_t grid = tile_grid(needles.tiles);
        SearchLevels<K> lv = {};
        lv.level[0] = (const K*) c.hay;
        lv.len[0] = p.len[0];
        for (uint32_t k = 1; k <= p.levels; k++)
        {
            lv.level[k] = (const K*) ((const char*) c.s->index.ptr + p.offset[k]);
            lv.len[k] = p.len[k];
        }
        lv.levels = p.levels;
        lv.xf = key_xf_of(c.key_type);
        hipLaunchKernelGGL((sorted_search_kernel<K, BOUNDS>), dim3(grid), dim3(kTileThreads), 0, c.stream, lv, needles, c.out_lower, c.out_upper);
    }
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

template<typename K>
glu_status launch_search(const Call& c, const SearchPlan& p, bool indexed)
{
    if (c.out_lower && c.out_upper) return launch_search<K, SEARCH_BOTH>(c, p, indexed);
    return c.out_lower ? launch_search<K, SEARCH_LOWER>(c, p, indexed) : launch_search<K, SEARCH_UPPER>(c, p, indexed);
}

void remember(glu_sorted_search_s* s, const void* hay, size_t hay_count, int key_type, uint32_t top)
{
    s->built.valid = true;
    s->built.hay = hay;
    s->built.hay_count = hay_count;
    s->built.key_type = key_type;
    s->built.top_entries = top;
}

// what index_ptr and run_ptr check of a haystack
glu_status check_hay(glu_sorted_search_s* s, const void* hay, size_t hay_count, int key_type)
{
    GLU_TRY(check_not_null(s, "search"));
    GLU_TRY(check_key_type(key_type));
    GLU_TRY(check_hay_count(hay_count));
    if (hay_count && !hay) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid hay buffer");
    GLU_TRY(check_aligned(hay, key_bytes_of(key_type), "hay", "the key size"));
    return check_top_entries(s->top_entries, key_bytes_of(key_type));
}

// ---- the batched search ------------------------------------------------------------------------------------------------------------
glu_status check_batch_window(uint64_t keys, uint32_t key_bytes)
{
    if (keys == kSearchBatchWindowUnset || search_batch_window_ok(keys, key_bytes)) return GLU_OK;
    return fail(GLU_ERROR_INVALID_ARGUMENT, "the batch window must be 0 or lie in [%u, %u] for %u-byte keys (got %llu)", kSearchBatchMinWindow,
                search_batch_max_window(key_bytes), key_bytes, (unsigned long long) keys);
}

// both forms behind their size checks.  hay_offsets NULL: equal partitions of hay_count keys; needle_offsets NULL: equal rows of
// needle_row needles.
struct BatchCall
{
    glu_sorted_search_s* s;
    const void* hay;
    size_t hay_total, hay_count;
    const uint32_t* hay_offsets;
    const void* needles;
    size_t needle_total, needle_row;
    const uint32_t* needle_offsets;
    size_t num_segments;
    int key_type;
    uint32_t* out_lower;
    uint32_t* out_upper;
    void* stream;
};

template<typename K, int BOUNDS>
void launch_batch(const SearchBatchArgs<K>& a, uint32_t grid, hipStream_t stream)
{
    if (a.needle_offsets)
        hipLaunchKernelGGL((sorted_search_batch_kernel<K, BOUNDS, true>), dim3(grid), dim3(kTileThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((sorted_search_batch_kernel<K, BOUNDS, false>), dim3(grid), dim3(kTileThreads), 0, stream, a);
}

template<typename K>
glu_status launch_batch(const BatchCall& c, uint32_t window)
{
    SearchBatchArgs<K> a = {};
    a.hay = (const K*) c.hay;
    a.hay_offsets = c.hay_offsets;
    a.needle_offsets = c.needle_offsets;
    a.out_lower = c.out_lower;
    a.out_upper = c.out_upper;
    a.needles = tile_span<K, kSearchBatchPacks>(c.needles, c.needle_total);
    a.rows = search_batch_make_rows((uint32_t) c.needle_row, (uint32_t) c.hay_count);
    a.hay_total = (uint32_t) c.hay_total;
    a.num_segments = (uint32_t) c.num_segments;
    a.window = window;
    a.xf = key_xf_of(c.key_type);
    const uint32_t grid = tile_grid(a.needles.tiles);
    const hipStream_t st = pick_stream(c.stream);
    if (c.out_lower && c.out_upper)
        launch_batch<K, SEARCH_BOTH>(a, grid, st);
    else if (c.out_lower)
        launch_batch<K, SEARCH_LOWER>(a, grid, st);
    else
        launch_batch<K, SEARCH_UPPER>(a, grid, st);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

glu_status run_batch(const BatchCall& c)
{
    const uint32_t kb = key_bytes_of(c.key_type);
    c.s->last = {(uint32_t) GLU_SEARCH_PATH_BATCH, 0u, 0u};
    if (!c.num_segments || !c.needle_total) return GLU_OK; // nothing to find: no array is looked at
    if (c.hay_total && !c.hay) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid hay buffer");
    if (!c.needles) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid needles buffer");
    if (!c.out_lower && !c.out_upper) return fail(GLU_ERROR_INVALID_ARGUMENT, "out_lower and out_upper are both NULL");
    GLU_TRY(check_aligned(c.hay, kb, "hay", "the key size"));
    GLU_TRY(check_aligned(c.needles, kb, "needles", "the key size"));
    GLU_TRY(check_aligned_4(c.out_lower, "out_lower"));
    GLU_TRY(check_aligned_4(c.out_upper, "out_upper"));
    GLU_TRY(check_aligned_4(c.hay_offsets, "hay_offsets"));
    GLU_TRY(check_aligned_4(c.needle_offsets, "needle_offsets"));
    const size_t out_bytes = c.needle_total * sizeof(uint32_t), offsets_bytes = (c.num_segments + 1) * sizeof(uint32_t);
    GLU_TRY(check_disjoint({{c.out_lower, out_bytes, "out_lower"}, {c.out_upper, out_bytes, "out_upper"}},
                           {{c.hay, c.hay_total * kb, "hay"},
                            {c.needles, c.needle_total * kb, "needles"},
                            {c.hay_offsets, offsets_bytes, "hay_offsets"},
                            {c.needle_offsets, offsets_bytes, "needle_offsets"}},
                           kOutputsAfterInputs));
    GLU_TRY(check_batch_window(c.s->batch_window, kb));
    const uint32_t window = search_batch_plan(c.needle_total, kb, c.s->batch_window).window;
    GLU_TRY(kb == 8 ? launch_batch<uint64_t>(c, window) : launch_batch<uint32_t>(c, window));
    c.s->last.kernels = 1;
    return GLU_OK;
}
} // namespace

extern "C" {

glu_status glu_sorted_search_plan_batch(size_t needle_total, glu_key_type key_type, uint32_t window_keys, uint32_t* tile, uint32_t* tiles,
                                        uint32_t* window_keys_used, uint32_t* kernels)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_below_2_32(needle_total, "needle_total"));
    const uint32_t kb = key_bytes_of((int) key_type);
    GLU_TRY(check_batch_window(window_keys, kb));
    const SearchBatchPlan p = search_batch_plan(needle_total, kb, window_keys);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(window_keys_used, p.window);
    store(kernels, p.kernels);
    return GLU_OK;
}

glu_status glu_sorted_search_set_batch_window(glu_sorted_search search, uint32_t keys)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    // the widest range here (4-byte keys end at 8192); a call holds it against its own key width
    if (keys != GLU_SEARCH_BATCH_WINDOW_DEFAULT && !search_batch_window_ok(keys, 4))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "the batch window must be 0 or lie in [%u, %u] (got %u)", kSearchBatchMinWindow,
                    search_batch_max_window(4), keys);
    search->batch_window = keys;
    return GLU_OK;
}

glu_status glu_sorted_search_run_batch_ptr(glu_sorted_search search, const void* hay, size_t hay_count, const void* needles, size_t needle_count,
                                           size_t num_partitions, glu_key_type key_type, uint32_t* out_lower, uint32_t* out_upper, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    GLU_TRY(check_key_type((int) key_type));
    const size_t most = ((size_t) 1 << 32) - 1;
    if (num_partitions > most || (hay_count && num_partitions > most / hay_count))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "hay_count * num_partitions must stay below 2^32 (got hay_count %zu, num_partitions %zu)", hay_count,
                    num_partitions);
    if (needle_count && num_partitions > most / needle_count)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "needle_count * num_partitions must stay below 2^32 (got needle_count %zu, num_partitions %zu)",
                    needle_count, num_partitions);
    return run_batch({search, hay, hay_count * num_partitions, hay_count, nullptr, needles, needle_count * num_partitions, needle_count, nullptr,
                      num_partitions, (int) key_type, out_lower, out_upper, stream});
}

glu_status glu_sorted_search_run_batch_offsets_ptr(glu_sorted_search search, const void* hay, size_t hay_total, const uint32_t* hay_offsets,
                                                   const void* needles, size_t needle_total, const uint32_t* needle_offsets, size_t num_segments,
                                                   glu_key_type key_type, uint32_t* out_lower, uint32_t* out_upper, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_total(hay_total));
    GLU_TRY(check_batch_total(needle_total));
    size_t needle_row = 0;
    if (num_segments && needle_total)
    {
        GLU_TRY(check_not_null(hay_offsets, "hay_offsets"));
        if (!needle_offsets)
        {
            if (needle_total % num_segments)
                return fail(GLU_ERROR_INVALID_ARGUMENT,
                            "needle_total must be a multiple of num_segments where needle_offsets is NULL (got needle_total %zu, num_segments %zu)",
                            needle_total, num_segments);
            needle_row = needle_total / num_segments;
        }
    }
    return run_batch({search, hay, hay_total, 0, hay_offsets, needles, needle_total, needle_row, needle_offsets, num_segments, (int) key_type,
                      out_lower, out_upper, stream});
}

glu_status glu_sorted_search_plan(size_t hay_count, size_t needle_count, glu_key_type key_type, uint32_t top_entries, uint32_t* path,
                                  uint32_t* levels, uint32_t* fanout, size_t* index_bytes)
{
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_hay_count(hay_count));
    GLU_TRY(check_needle_count(needle_count));
    const uint32_t kb = key_bytes_of((int) key_type);
    GLU_TRY(check_top_entries(top_entries, kb));
    const SearchPlan p = search_plan(hay_count, kb, top_entries_of(top_entries, kb));
    store(path, pick_path(GLU_SEARCH_PATH_AUTO, p, hay_count, needle_count));
    store(levels, p.levels);
    store(fanout, p.fanout);
    store(index_bytes, p.index_bytes);
    return GLU_OK;
}

glu_status glu_sorted_search_create(glu_sorted_search* out) { return create_object(out); }

glu_status glu_sorted_search_destroy(glu_sorted_search search) { return destroy_object(search); }

glu_status glu_sorted_search_prepare(glu_sorted_search search, size_t hay_count, glu_key_type key_type)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    GLU_TRY(check_key_type((int) key_type));
    GLU_TRY(check_hay_count(hay_count));
    const uint32_t kb = key_bytes_of((int) key_type);
    GLU_TRY(check_top_entries(search->top_entries, kb));
    return reserve_index(search, search_plan(hay_count, kb, top_entries_of(search->top_entries, kb)));
}

glu_status glu_sorted_search_set_option(glu_sorted_search search, const char* name, long long value)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    GLU_TRY(check_not_null(name, "name"));
    if (!strcmp(name, "PATH"))
    {
        if (value < GLU_SEARCH_PATH_AUTO || value > GLU_SEARCH_PATH_INDEXED)
            return fail(GLU_ERROR_INVALID_ARGUMENT, "PATH must be GLU_SEARCH_PATH_AUTO, _DIRECT or _INDEXED (0 .. 2) (got %lld)", value);
        search->path = (int) value;
        return GLU_OK;
    }
    if (!strcmp(name, "TOP_ENTRIES"))
    {
        // the widest range here (8-byte keys start at 16, 4-byte keys end at 8192); a call holds it against its own key width
        if (value < (long long) search_fanout(8) || value > (long long) search_lds_entries(4))
            return fail(GLU_ERROR_INVALID_ARGUMENT, "TOP_ENTRIES must lie in [%u, %u] (got %lld)", search_fanout(8), search_lds_entries(4), value);
        search->top_entries = (uint32_t) value;
        return GLU_OK;
    }
    return fail(GLU_ERROR_INVALID_ARGUMENT, "Unknown option: %s (the options are PATH and TOP_ENTRIES)", name);
}

glu_status glu_sorted_search_index_ptr(glu_sorted_search search, const void* hay, size_t hay_count, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_hay(search, hay, hay_count, (int) key_type));
    const uint32_t kb = key_bytes_of((int) key_type), top = top_entries_of(search->top_entries, kb);
    const SearchPlan p = search_plan(hay_count, kb, top);
    GLU_TRY(reserve_index(search, p));
    search->last = {GLU_SEARCH_PATH_INDEXED, p.levels, 0u};
    if (p.levels)
    {
        GLU_TRY(kb == 8 ? launch_index<uint64_t>(search, p, hay, (int) key_type, pick_stream(stream))
                        : launch_index<uint32_t>(search, p, hay, (int) key_type, pick_stream(stream)));
        search->last.kernels = 1;
    }
    remember(search, hay, hay_count, (int) key_type, top);
    return GLU_OK;
}

glu_status glu_sorted_search_run_ptr(glu_sorted_search search, const void* hay, size_t hay_count, const void* needles, size_t needle_count,
                                     glu_key_type key_type, uint32_t* out_lower, uint32_t* out_upper, int reuse_index, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_hay(search, hay, hay_count, (int) key_type));
    GLU_TRY(check_needle_count(needle_count));
    const uint32_t kb = key_bytes_of((int) key_type), top = top_entries_of(search->top_entries, kb);
    if (needle_count && !needles) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid needles buffer");
    if (!out_lower && !out_upper) return fail(GLU_ERROR_INVALID_ARGUMENT, "out_lower and out_upper are both NULL");
    GLU_TRY(check_aligned(needles, kb, "needles", "the key size"));
    GLU_TRY(check_aligned_4(out_lower, "out_lower"));
    GLU_TRY(check_aligned_4(out_upper, "out_upper"));
    const size_t out_bytes = needle_count * sizeof(uint32_t);
    GLU_TRY(check_disjoint({{out_lower, out_bytes, "out_lower"}, {out_upper, out_bytes, "out_upper"}},
                           {{hay, hay_count * kb, "hay"}, {needles, needle_count * kb, "needles"}}, kOutputsAfterInputs));

    const SearchPlan p = search_plan(hay_count, kb, top);
    bool indexed;
    if (reuse_index)
    {
        const auto& b = search->built;
        if (!b.valid) return fail(GLU_ERROR_INVALID_STATE, "reuse_index: no index has been built (glu_sorted_search_index_ptr)");
        if (b.hay != hay || b.hay_count != hay_count || b.key_type != (int) key_type || b.top_entries != top)
            return fail(GLU_ERROR_INVALID_STATE, "reuse_index: the index was built for another hay, hay_count, key type or TOP_ENTRIES");
        indexed = p.levels != 0;
    }
    else
    {
        indexed = pick_path(search->path, p, hay_count, needle_count) == GLU_SEARCH_PATH_INDEXED;
        if (indexed) GLU_TRY(reserve_index(search, p));
    }
    const hipStream_t st = pick_stream(stream);
    search->last = {(uint32_t) (indexed ? GLU_SEARCH_PATH_INDEXED : GLU_SEARCH_PATH_DIRECT), indexed ? p.levels : 0u, 0u};
    if (indexed && !reuse_index)
    {
        GLU_TRY(kb == 8 ? launch_index<uint64_t>(search, p, hay, (int) key_type, st) : launch_index<uint32_t>(search, p, hay, (int) key_type, st));
        search->last.kernels++;
        remember(search, hay, hay_count, (int) key_type, top);
    }
    if (!needle_count) return GLU_OK;
    const Call c{search, hay, hay_count, needles, needle_count, (int) key_type, out_lower, out_upper, st};
    GLU_TRY(kb == 8 ? launch_search<uint64_t>(c, p, indexed) : launch_search<uint32_t>(c, p, indexed));
    search->last.kernels++;
    return GLU_OK;
}

glu_status glu_sorted_search_last(glu_sorted_search search, uint32_t* path, uint32_t* levels, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(search, "search"));
    store(path, search->last.path);
    store(levels, search->last.levels);
    store(kernels, search->last.kernels);
    return GLU_OK;
}

} // extern "C"
