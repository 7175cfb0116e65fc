// glu_histogram.hip -- histogram of libglu_hip.so (histogram_kernels.hpp): glu_histogram_create, glu_histogram_destroy,
// glu_histogram_prepare, glu_histogram_run_even_ptr, glu_histogram_run_edges_ptr, glu_histogram_plan, glu_histogram_last.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include "glu_histogram_object.hpp"
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

template<typename T>
glu_status run_edges(glu_histogram_s* h, const void* samples, size_t count, const void* edges, uint32_t bins, uint32_t* out_counts, bool accumulate,
                     hipStream_t stream)
{
    HistEdges<T> rule;
    rule.edges = (const T*) edges;
    rule.n_edges = bins + 1;
    rule.steps = hist_steps(rule.n_edges);
    return enqueue<T, HistEdges<T>, HIST_EDGES>(h, samples, count, rule, bins, out_counts, accumulate, stream);
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
        return is_signed ? enqueue<int32_t, HistEvenInt, HIST_EVEN>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st)
                         : enqueue<uint32_t, HistEvenInt, HIST_EVEN>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st);
    }
    const bool wide = key_type == GLU_KEY_FLOAT64;
    const double l = wide ? *(const double*) lo : (double) *(const float*) lo, u = wide ? *(const double*) hi : (double) *(const float*) hi;
    HistEvenFloat rule;
    if (!hist_make_even_float(l, u, nb, &rule))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "lo and hi must be finite with lo < hi, and hi - lo and bins / (hi - lo) finite in double (lo %g, hi %g)",
                    l, u);
    return wide ? enqueue<double, HistEvenFloat, HIST_EVEN>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st)
                : enqueue<float, HistEvenFloat, HIST_EVEN>(histogram, samples, count, rule, nb, out_counts, accumulate != 0, st);
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
    const bool acc = accumulate != 0;
    switch (key_type)
    {
    case GLU_KEY_UINT32: return run_edges<uint32_t>(histogram, samples, count, edges, nb, out_counts, acc, st);
    case GLU_KEY_INT32: return run_edges<int32_t>(histogram, samples, count, edges, nb, out_counts, acc, st);
    case GLU_KEY_FLOAT32: return run_edges<float>(histogram, samples, count, edges, nb, out_counts, acc, st);
    case GLU_KEY_UINT64: return run_edges<uint64_t>(histogram, samples, count, edges, nb, out_counts, acc, st);
    case GLU_KEY_INT64: return run_edges<int64_t>(histogram, samples, count, edges, nb, out_counts, acc, st);
    default: return run_edges<double>(histogram, samples, count, edges, nb, out_counts, acc, st);
    }
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

} // extern "C"
