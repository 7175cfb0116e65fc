// glu_sorted_search.hip -- sorted search of libglu_hip.so (sorted_search_kernels.hpp): glu_sorted_search_create,
// glu_sorted_search_destroy, glu_sorted_search_prepare, glu_sorted_search_set_option, glu_sorted_search_index_ptr,
// glu_sorted_search_run_ptr, glu_sorted_search_plan, glu_sorted_search_last.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "glu_sorted_search_object.hpp"
#include "sorted_search_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

static_assert(kSearchLevelsMax == kSearchMaxLevels, "the host's level rule fills the kernels' level table");

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
} // namespace

extern "C" {

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
