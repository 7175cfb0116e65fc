// glu_histogram.hip -- histogram of libglu_hip.so (histogram_kernels.hpp): glu_histogram_create, glu_histogram_destroy,
// glu_histogram_prepare, glu_histogram_run_even_ptr, glu_histogram_run_edges_ptr, glu_histogram_plan, glu_histogram_last; and the
// batched histogram (histogram_batch_kernels.hpp over histogram_batch_walk.hpp): glu_histogram_run_batch_even_ptr,
// _run_batch_offsets_even_ptr, _run_batch_edges_ptr, _run_batch_offsets_edges_ptr, _prepare_batch, _plan_batch, _read_batch.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include "glu_histogram_object.hpp"
#include "histogram_batch_kernels.hpp"
#include "histogram_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// what both entry points and the plan check of the counts: the key type, count, bins against the limit of the mode
glu_status check_counts(size_t count, size_t bins, int key_type, int mode)
{
    GLU_TRY(check_key_type(key_type));
    if (mode != HIST_EVEN && mode != HIST_EDGES) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid mode: %d (GLU_HISTOGRAM_EVEN or _EDGES)", mode);
    GLU_TRY(check_tile_count(count, "histogram takes a count below 2^32"));
    const size_t most = mode == HIST_EVEN ? kHistMaxEvenBins : kHistLdsBins;
    if (bins < 1 || bins > most)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "bins must be 1 .. %zu for %s (got %zu)%s", most, mode == HIST_EVEN ? "even bins" : "edges", bins,
                    mode == HIST_EDGES && bins > most ? ": sort the samples, search the edges in them and difference the bounds" : "");
    if (mode == HIST_EVEN && (key_type == (int) GLU_KEY_UINT64 || key_type == (int) GLU_KEY_INT64))
        return fail(GLU_ERROR_INVALID_ARGUMENT,
                    "key type %d has no even bins (they are not exact in double): pass the edges to glu_histogram_run_edges_ptr", key_type);
    return GLU_OK;
}

// samples, out_counts and (edges mode) edges: NULL, alignment, overlap.  `count` == 0: the samples are not looked at.
glu_status check_arrays(const void* samples, size_t count, uint32_t kb, const void* edges, bool with_edges, size_t bins, const uint32_t* out_counts)
{
    if (count && !samples) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid samples buffer");
    if (!out_counts) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid out_counts buffer");
    if (with_edges && !edges) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid edges buffer");
    if (count) GLU_TRY(check_aligned(samples, kb, "samples", "the sample size"));
    GLU_TRY(check_aligned_4(out_counts, "out_counts"));
    if (with_edges) GLU_TRY(check_aligned(edges, kb, "edges", "the sample size"));
    return check_disjoint({{out_counts, bins * sizeof(uint32_t), "out_counts"}},
                          {{samples, count * kb, "samples"}, {with_edges ? edges : nullptr, (bins + 1) * kb, "edges"}});
}

// the samples as the 16-byte packs from the boundary at or below them, in tiles of `tile` elements
// (tile_span<T, PACKS>() of tile_span.hpp states the same base, lo and hi, but counts tiles of 256 threads; the workgroups here have
// 256, 512 or 1024, so the tiles are counted with the plan's tile)
template<typename T>
TileSpan<T> hist_span(const void* samples, size_t count, uint32_t tile)
{
    TileSpan<T> s;
    s.lo = ((uintptr_t) samples & 15u) / sizeof(T);
    s.hi = s.lo + count;
    s.base = (const T*) samples - s.lo;
    s.tiles = count ? (uint32_t) ((s.hi + tile - 1) / tile) : 0u; // (one more than the plan's at the most)
    return s;
}

template<typename T, typename Rule, int MODE>
glu_status enqueue(glu_histogram_s* h, const void* samples, size_t count, const Rule& rule, uint32_t bins, uint32_t* out_counts, bool accumulate,
                   hipStream_t stream)
{
    constexpr uint32_t THREADS = hist_threads(sizeof(T), MODE);
    const HistPlan p = hist_plan(count, bins, sizeof(T), MODE, accumulate);
    h->last = {p.path, p.groups, p.kernels};
    HistArgs<T, Rule> a = {};
    a.samples = hist_span<T>(samples, count, p.tile);
    a.rule = rule;
    a.bins = bins;
    if (p.path == HIST_PATH_LDS)
    {
        if (count)
        {
            GLU_TRY(h->partial.reserve(p.scratch_bytes));
            a.dst = (uint32_t*) h->partial.ptr;
            hipLaunchKernelGGL((histogram_count_kernel<T, Rule, THREADS>), dim3(p.groups), dim3(THREADS), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (count || !accumulate)
        {
            hipLaunchKernelGGL(histogram_sum_kernel, dim3((bins + kHistSumCols - 1) / kHistSumCols), dim3(kHistSumThreads), 0, stream,
                               (const uint32_t*) h->partial.ptr, p.groups, bins, out_counts, accumulate ? 1u : 0u);
            HIP_TRY(hipGetLastError());
        }
        return GLU_OK;
    }
    if constexpr (MODE == HIST_EVEN)
    {
        if (!accumulate)
        {
            hipLaunchKernelGGL(histogram_clear_kernel, dim3((bins + kHistClearThreads - 1) / kHistClearThreads), dim3(kHistClearThreads), 0, stream,
                               out_counts, bins);
            HIP_TRY(hipGetLastError());
        }
        if (count)
        {
            a.dst = out_counts;
            hipLaunchKernelGGL((histogram_global_kernel<T, Rule, THREADS>), dim3(p.groups), dim3(THREADS), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        return GLU_OK;
    }
    return fail(GLU_ERROR_INVALID_ARGUMENT, "edges take at most %u bins", kHistLdsBins); // (check_counts refused it already)
}

// The rule of even bins from the host's lo and hi, for the single and the batched call alike: run(a value of the sample's type, the
// rule), or the invalid argument that lo, hi and bins are.  (64-bit integers: check_counts refused them already.)
template<typename Run>
glu_status with_even_rule(glu_key_type key_type, const void* lo, const void* hi, uint32_t nb, Run run)
{
    if (key_type == GLU_KEY_UINT32 || key_type == GLU_KEY_INT32)
    {
        const bool is_signed = key_type == GLU_KEY_INT32;
        const int64_t l = is_signed ? (int64_t) * (const int32_t*) lo : (int64_t) * (const uint32_t*) lo;
        const int64_t u = is_signed ? (int64_t) * (const int32_t*) hi : (int64_t) * (const uint32_t*) hi;
        HistEvenInt rule;
        if (!hist_make_even_int(l, u, nb, &rule))
            return fail(GLU_ERROR_INVALID_ARGUMENT,
                        "(hi - lo) / bins must be a whole number >= 1 for integer samples (lo %lld, hi %lld, bins %u): pass the edges to "
                        "glu_histogram_run_edges_ptr",
                        (long long) l, (long long) u, nb);
        return is_signed ? run(int32_t(), rule) : run(uint32_t(), rule);
    }
    const bool wide = key_type == GLU_KEY_FLOAT64;
    const double l = wide ? *(const double*) lo : (double) *(const float*) lo, u = wide ? *(const double*) hi : (double) *(const float*) hi;
    HistEvenFloat rule;
    if (!hist_make_even_float(l, u, nb, &rule))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "lo and hi must be finite with lo < hi, and hi - lo and bins / (hi - lo) finite in double (lo %g, hi %g)",
                    l, u);
    return wide ? run(double(), rule) : run(float(), rule);
}

// ... and of the bins + 1 device edges
template<typename Run>
glu_status with_edges_rule(glu_key_type key_type, const void* edges, uint32_t nb, Run run)
{
    const auto typed = [&](auto sample) {
        using T = decltype(sample);
        HistEdges<T> rule;
        rule.edges = (const T*) edges;
        rule.n_edges = nb + 1;
        rule.steps = hist_steps(rule.n_edges);
        return run(sample, rule);
    };
    switch (key_type)
    {
    case GLU_KEY_UINT32: return typed(uint32_t());
    case GLU_KEY_INT32: return typed(int32_t());
    case GLU_KEY_FLOAT32: return typed(float());
    case GLU_KEY_UINT64: return typed(uint64_t());
    case GLU_KEY_INT64: return typed(int64_t());
    default: return typed(double());
    }
}

// ---- the batched call ---------------------------------------------------------------------------------------------------------
// what the four entry points and the plan check of the counts: `samples` is a segment's count (the plan) or the batch's total
glu_status check_batch_counts(size_t samples, size_t bins, int key_type, int mode)
{
    GLU_TRY(check_key_type(key_type));
    if (mode != HIST_EVEN && mode != HIST_EDGES) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid mode: %d (GLU_HISTOGRAM_EVEN or _EDGES)", mode);
    GLU_TRY(check_batch_total(samples));
    if (bins < 1 || bins > kHistLdsBins)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "bins must be 1 .. %u for a batched histogram (got %zu): every table is kept in LDS", kHistLdsBins, bins);
    if (mode == HIST_EVEN && (key_type == (int) GLU_KEY_UINT64 || key_type == (int) GLU_KEY_INT64))
        return fail(GLU_ERROR_INVALID_ARGUMENT,
                    "key type %d has no even bins (they are not exact in double): pass the edges to glu_histogram_run_batch_edges_ptr", key_type);
    return GLU_OK;
}

struct BatchCall
{
    glu_histogram_s* h;
    const void* samples;
    size_t count, num_segments, total; // equal partitions: count x num_segments; device offsets: total, num_segments
    const uint32_t* offsets;
    uint32_t bins;
    uint32_t* out_counts;
    bool accumulate;
    hipStream_t stream;
};

// samples, offsets, out_counts and (edges mode) edges of a batch: NULL, alignment, overlap.  What is never read may be NULL.
glu_status check_batch_arrays(const BatchCall& c, uint32_t kb, const void* edges, bool with_edges)
{
    const size_t read = c.num_segments ? c.total : 0; // samples that can be read
    if (read && !c.samples) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid samples buffer");
    if (c.num_segments && !c.out_counts) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid out_counts buffer");
    if (with_edges && read && !edges) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid edges buffer");
    if (read) GLU_TRY(check_aligned(c.samples, kb, "samples", "the sample size"));
    GLU_TRY(check_aligned_4(c.out_counts, "out_counts"));
    if (with_edges) GLU_TRY(check_aligned(edges, kb, "edges", "the sample size"));
    return check_disjoint({{c.out_counts, c.num_segments * c.bins * sizeof(uint32_t), "out_counts"}},
                          {{c.samples, read * kb, "samples"},
                           {with_edges ? edges : nullptr, ((size_t) c.bins + 1) * kb, "edges"},
                           {c.offsets, c.offsets ? (c.num_segments + 1) * sizeof(uint32_t) : 0, "offsets"}});
}

// workgroups of the kernels that walk a list of up to `entries` entries: a few to the CU, each taking the entries g, g + grid, ...
inline uint32_t batch_grid(uint64_t entries) { return (uint32_t) std::min<uint64_t>(std::max<uint64_t>(entries, 1), cus() * 8u); }

template<typename T, typename Rule, int MODE>
glu_status enqueue_batch(const BatchCall& c, const Rule& rule)
{
    constexpr uint32_t THREADS = hist_threads(sizeof(T), MODE);
    glu_histogram_s* h = c.h;
    HistBatchArgs<T, Rule> a = {};
    a.samples = (const T*) c.samples;
    a.rule = rule;
    a.bins = c.bins;
    a.accumulate = c.accumulate ? 1u : 0u;
    a.out = c.out_counts;
    a.l.nsegs = (uint32_t) c.num_segments;
    const uint32_t sum_cols = (c.bins + kHistSumCols - 1) / kHistSumCols;
    const size_t row_bytes = (size_t) c.bins * sizeof(uint32_t);
    uint32_t kernels = 0;
    h->last_batch.reset();
    h->last = {HIST_PATH_BATCH, 0, 0};
    if (!c.offsets) // equal partitions: the host picks the class
    {
        const HistBatchPlan p = hist_batch_plan(c.count, c.bins, sizeof(T));
        a.l.count = c.count;
        a.l.layout.chunk = p.chunk;
        if (p.path) h->last_batch.by_class[p.path - 1] = a.l.nsegs;
        if (p.path == 0)
        {
            if (!c.accumulate)
            {
                const uint64_t n = (uint64_t) c.num_segments * c.bins;
                hipLaunchKernelGGL(histogram_batch_clear_kernel, dim3(batch_grid((n + 255) / 256)), dim3(256), 0, c.stream, c.out_counts, n);
                kernels++;
            }
        }
        else if (p.path == 1)
        {
            hipLaunchKernelGGL((histogram_batch_wave_kernel<T, Rule>), dim3(batch_grid((c.num_segments + kHistBatchWaves - 1) / kHistBatchWaves)),
                               dim3(256), 0, c.stream, a);
            kernels++;
        }
        else if (p.path == 2)
        {
            hipLaunchKernelGGL((histogram_batch_block_kernel<T, Rule, THREADS>), dim3(batch_grid(c.num_segments)), dim3(THREADS), 0, c.stream, a, 0u,
                               (uint64_t) c.num_segments);
            kernels++;
        }
        else
        {
            const uint64_t items = (uint64_t) p.workgroups * c.num_segments; // (below 2^32 / chunk + 2^24)
            GLU_TRY(h->batch_partial.reserve(items * row_bytes));
            a.partial = (uint32_t*) h->batch_partial.ptr;
            a.l.chunks_per = p.workgroups;
            hipLaunchKernelGGL((histogram_batch_block_kernel<T, Rule, THREADS>), dim3(batch_grid(items)), dim3(THREADS), 0, c.stream, a, 1u, items);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(histogram_batch_sum_kernel, dim3(sum_cols, std::min<uint32_t>(a.l.nsegs, 65535u)), dim3(kHistSumThreads), 0, c.stream,
                               a.l, (const uint32_t*) a.partial, c.out_counts, c.bins, a.accumulate);
            kernels += 2;
        }
        HIP_TRY(hipGetLastError());
        h->last.kernels = kernels;
        return GLU_OK;
    }
    // device offsets: the counts cleared, binning, then a kernel for the wave list, one for the block list and two for the long
    // segments, each only where the counts the host was given leave its list any room: at most five kernels whatever the data hold
    uint32_t *counts, *lists, bin_grid;
    GLU_TRY(begin_batch_offsets(h->batch_lists, hist_batch_classes(c.bins, sizeof(T)), c.total, c.num_segments, c.stream, a.l.layout, counts, lists,
                                bin_grid));
    const BatchListsLayout& layout = a.l.layout;
    GLU_TRY(h->batch_partial.reserve((size_t) layout.capacity[BATCH_LIST_CHUNKS] * row_bytes));
    a.partial = (uint32_t*) h->batch_partial.ptr;
    a.l.offsets = c.offsets;
    a.l.total = (uint32_t) c.total;
    a.l.counts = counts;
    a.l.lists = lists;
    hipLaunchKernelGGL(histogram_batch_bin_kernel, dim3(bin_grid), dim3(256), 0, c.stream, a.l, counts, lists, c.out_counts, c.bins, a.accumulate);
    HIP_TRY(hipGetLastError());
    kernels++;
    h->last_batch.on_device = true;
    if (c.total) // (else every segment is empty)
    {
        if (layout.limit[BATCH_LIST_SHORT4] && layout.capacity[BATCH_LIST_SHORT4]) // (no wave class with more than 2048 bins)
        {
            hipLaunchKernelGGL((histogram_batch_wave_kernel<T, Rule>),
                               dim3(batch_grid(((uint64_t) layout.capacity[BATCH_LIST_SHORT4] + kHistBatchWaves - 1) / kHistBatchWaves)), dim3(256), 0,
                               c.stream, a);
            HIP_TRY(hipGetLastError());
            kernels++;
        }
        if (layout.capacity[BATCH_LIST_BLOCK])
        {
            hipLaunchKernelGGL((histogram_batch_block_kernel<T, Rule, THREADS>), dim3(batch_grid(layout.capacity[BATCH_LIST_BLOCK])), dim3(THREADS), 0,
                               c.stream, a, 0u, (uint64_t) 0);
            HIP_TRY(hipGetLastError());
            kernels++;
        }
        if (layout.capacity[BATCH_LIST_LONG])
        {
            hipLaunchKernelGGL((histogram_batch_block_kernel<T, Rule, THREADS>), dim3(batch_grid(layout.capacity[BATCH_LIST_CHUNKS])), dim3(THREADS), 0,
                               c.stream, a, 1u, (uint64_t) 0);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(histogram_batch_sum_kernel, dim3(sum_cols, std::min<uint32_t>(layout.capacity[BATCH_LIST_LONG], 65535u)),
                               dim3(kHistSumThreads), 0, c.stream, a.l, (const uint32_t*) a.partial, c.out_counts, c.bins, a.accumulate);
            HIP_TRY(hipGetLastError());
            kernels += 2;
        }
    }
    h->last.kernels = kernels;
    return GLU_OK;
}

// the checks the four entry points share, then the rule and the call.  offsets == NULL: equal partitions of `count` samples
glu_status run_batch(glu_histogram_s* h, const void* samples, size_t count, size_t total, const uint32_t* offsets, bool with_offsets, size_t num_segments,
                     glu_key_type key_type, int mode, const void* lo, const void* hi, const void* edges, size_t bins, uint32_t* out_counts,
                     int accumulate, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(h, "histogram"));
    GLU_TRY(check_batch_segments(num_segments));
    if (!with_offsets)
    {
        if (count && num_segments > ((size_t) -1) / count) return fail(GLU_ERROR_INVALID_ARGUMENT, "count * num_partitions overflows");
        total = count * num_segments;
    }
    GLU_TRY(check_batch_counts(total, bins, (int) key_type, mode));
    if (mode == HIST_EVEN)
    {
        GLU_TRY(check_not_null(lo, "lo"));
        GLU_TRY(check_not_null(hi, "hi"));
    }
    const BatchCall c = {h, samples, count, num_segments, total, with_offsets ? offsets : nullptr, (uint32_t) bins, out_counts, accumulate != 0,
                         pick_stream(stream)};
    GLU_TRY(check_batch_arrays(c, key_bytes_of((int) key_type), edges, mode == HIST_EDGES));
    if (with_offsets) GLU_TRY(check_batch_offsets(offsets, num_segments));
    if (mode == HIST_EVEN) // (the rule is checked whatever the batch holds, as in the single call)
    {
        if (num_segments == 0) return with_even_rule(key_type, lo, hi, c.bins, [&](auto, const auto&) { return h->last_batch.reset(), GLU_OK; });
        return with_even_rule(key_type, lo, hi, c.bins, [&](auto sample, const auto& rule) {
            return enqueue_batch<decltype(sample), std::decay_t<decltype(rule)>, HIST_EVEN>(c, rule);
        });
    }
    if (num_segments == 0) return h->last_batch.reset(), GLU_OK;
    return with_edges_rule(key_type, edges, c.bins, [&](auto sample, const auto& rule) {
        return enqueue_batch<decltype(sample), HistEdges<decltype(sample)>, HIST_EDGES>(c, rule);
    });
}
} // namespace

extern "C" {

glu_status glu_histogram_plan(size_t count, size_t bins, glu_key_type key_type, int mode, uint32_t* path, uint32_t* threads, uint32_t* tile,
                              uint32_t* groups, uint32_t* kernels, size_t* scratch_bytes)
{
    GLU_TRY(check_counts(count, bins, (int) key_type, mode));
    const HistPlan p = hist_plan(count, (uint32_t) bins, key_bytes_of((int) key_type), mode, false);
    store(path, p.path);
    store(threads, p.threads);
    store(tile, p.tile);
    store(groups, p.groups);
    store(kernels, p.kernels);
    store(scratch_bytes, p.scratch_bytes);
    return GLU_OK;
}

glu_status glu_histogram_create(glu_histogram* out) { return create_object(out); }

glu_status glu_histogram_destroy(glu_histogram histogram) { return destroy_object(histogram); }

glu_status glu_histogram_prepare(glu_histogram histogram, size_t count, size_t bins)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    GLU_TRY(check_counts(count, bins, (int) GLU_KEY_UINT32, HIST_EVEN));
    return histogram->partial.reserve(hist_scratch_most(count, (uint32_t) bins));
}

glu_status glu_histogram_run_even_ptr(glu_histogram histogram, const void* samples, size_t count, glu_key_type key_type, const void* lo,
                                      const void* hi, size_t bins, uint32_t* out_counts, int accumulate, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    GLU_TRY(check_counts(count, bins, (int) key_type, HIST_EVEN));
    GLU_TRY(check_not_null(lo, "lo"));
    GLU_TRY(check_not_null(hi, "hi"));
    GLU_TRY(check_arrays(samples, count, 4u * (key_type == GLU_KEY_FLOAT64 ? 2u : 1u), nullptr, false, bins, out_counts));
    const hipStream_t st = pick_stream(stream);
    const uint32_t nb = (uint32_t) bins;
    return with_even_rule(key_type, lo, hi, nb, [&](auto sample, const auto& rule) {
        using T = decltype(sample);
        using Rule = std::decay_t<decltype(rule)>;
        return enqueue<T, Rule, HIST_EVEN>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st);
    });
}

glu_status glu_histogram_run_edges_ptr(glu_histogram histogram, const void* samples, size_t count, glu_key_type key_type, const void* edges,
                                       size_t bins, uint32_t* out_counts, int accumulate, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    GLU_TRY(check_counts(count, bins, (int) key_type, HIST_EDGES));
    GLU_TRY(check_arrays(samples, count, key_bytes_of((int) key_type), edges, true, bins, out_counts));
    const hipStream_t st = pick_stream(stream);
    const uint32_t nb = (uint32_t) bins;
    return with_edges_rule(key_type, edges, nb, [&](auto sample, const auto& rule) {
        using T = decltype(sample);
        return enqueue<T, HistEdges<T>, HIST_EDGES>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st);
    });
}

glu_status glu_histogram_last(glu_histogram histogram, uint32_t* path, uint32_t* groups, uint32_t* kernels)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    store(path, histogram->last.path);
    store(groups, histogram->last.groups);
    store(kernels, histogram->last.kernels);
    return GLU_OK;
}

glu_status glu_histogram_plan_batch(size_t count, size_t bins, glu_key_type key_type, int mode, uint32_t* path, uint32_t* workgroups,
                                    uint32_t* class_limits, uint32_t* chunk, size_t* scratch_bytes_per_chunk)
{
    GLU_TRY(check_batch_counts(count, bins, (int) key_type, mode));
    const HistBatchPlan p = hist_batch_plan(count, (uint32_t) bins, key_bytes_of((int) key_type));
    store(path, p.path);
    store(workgroups, p.workgroups);
    if (class_limits)
    {
        class_limits[0] = p.wave_limit;
        class_limits[1] = p.block_limit;
    }
    store(chunk, p.chunk);
    store(scratch_bytes_per_chunk, p.scratch_bytes_per_chunk);
    return GLU_OK;
}

glu_status glu_histogram_prepare_batch(glu_histogram histogram, size_t total, size_t num_segments, size_t bins)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    GLU_TRY(check_batch_segments(num_segments));
    GLU_TRY(check_batch_counts(total, bins, (int) GLU_KEY_UINT32, HIST_EVEN));
    for (uint32_t key_bytes = 4; key_bytes <= 8; key_bytes += 4) // (the most either key width takes; the scratch only grows)
    {
        BatchListsLayout layout;
        GLU_TRY(reserve_batch_lists(histogram->batch_lists, hist_batch_classes((uint32_t) bins, key_bytes), total, num_segments, layout));
        GLU_TRY(histogram->batch_partial.reserve((size_t) hist_batch_slots(total, num_segments, layout.limit[BATCH_LIST_BLOCK], layout.chunk) * bins * sizeof(uint32_t)));
    }
    return GLU_OK;
}

glu_status glu_histogram_run_batch_even_ptr(glu_histogram histogram, const void* samples, size_t count, size_t num_partitions,
                                            glu_key_type key_type, const void* lo, const void* hi, size_t bins, uint32_t* out_counts, int accumulate,
                                            void* stream)
{
    return run_batch(histogram, samples, count, 0, nullptr, false, num_partitions, key_type, HIST_EVEN, lo, hi, nullptr, bins, out_counts, accumulate,
                     stream);
}

glu_status glu_histogram_run_batch_offsets_even_ptr(glu_histogram histogram, const void* samples, size_t total, const uint32_t* offsets,
                                                    size_t num_segments, glu_key_type key_type, const void* lo, const void* hi, size_t bins,
                                                    uint32_t* out_counts, int accumulate, void* stream)
{
    return run_batch(histogram, samples, 0, total, offsets, true, num_segments, key_type, HIST_EVEN, lo, hi, nullptr, bins, out_counts, accumulate,
                     stream);
}

glu_status glu_histogram_run_batch_edges_ptr(glu_histogram histogram, const void* samples, size_t count, size_t num_partitions,
                                             glu_key_type key_type, const void* edges, size_t bins, uint32_t* out_counts, int accumulate, void* stream)
{
    return run_batch(histogram, samples, count, 0, nullptr, false, num_partitions, key_type, HIST_EDGES, nullptr, nullptr, edges, bins, out_counts,
                     accumulate, stream);
}

glu_status glu_histogram_run_batch_offsets_edges_ptr(glu_histogram histogram, const void* samples, size_t total, const uint32_t* offsets,
                                                     size_t num_segments, glu_key_type key_type, const void* edges, size_t bins,
                                                     uint32_t* out_counts, int accumulate, void* stream)
{
    return run_batch(histogram, samples, 0, total, offsets, true, num_segments, key_type, HIST_EDGES, nullptr, nullptr, edges, bins, out_counts,
                     accumulate, stream);
}

glu_status glu_histogram_read_batch(glu_histogram histogram, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(histogram, "histogram"));
    return histogram->last_batch.read(histogram->batch_lists, 1, wave_segments, block_segments, long_segments); // (list 0 is the wave class)
}

} // extern "C"
