// glu_sort_placement.hip -- the placement search of libglu_hip.so: where the large scratch arrays of a sort lie to each other, chosen
// by measurement (tune_scratch_placement for sort_prepare, place_pair_by_measurement for glu_dist_prepare).  It sorts through
// glu_sort_driver.hpp and launches one kernel of its own, the fill of the calibration arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "glu_host.hpp"
#include "glu_sort_driver.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// Placement of the two large scratch arrays by measurement (sort_prepare).  Two 1 GiB arrays that hipMalloc hands out one
// after the other lie 1 GiB + 2 MiB apart, and whether the key scratch and the value scratch then collide in the memory
// system is a property of where they fell, the same for every caller array the sort is later given (tools/placement_scratch.py,
// profiles/r03/placement_scratch_spacers.txt: of eight sorter objects in one process the same three sort every caller pair
// in 3.76-3.80 ms and the others in 3.9-4.05 ms).  User space cannot choose physical pages, but it can choose among
// allocations: the value array is allocated behind spacers of 0 .. 6 GiB, every candidate sorts a scratch copy of
// pseudo-random pairs twice (events on the library queue), the fastest pair of arrays is kept and everything else freed.
// One-off, and only inside the explicit prepare entry points (glu_radix_sort_prepare*, glu_dist_prepare; the reference's
// prepare_internal_buffers is where its allocations happen too).  A sort on an object that was not prepared for its size
// grows the scratch with two plain hipMallocs and reports zero candidates.  GLU_HIP_SCRATCH_TUNE=0 switches it off.
__global__ void tune_fill_kernel(uint32_t* __restrict__ p, size_t words, uint32_t salt)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t) gridDim.x * blockDim.x)
    {
        uint32_t x = (uint32_t) i * 2654435761u + salt;
        x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
        p[i] = x;
    }
}

// What the two callers of the search differ in (the fourth difference, what happens when nothing was chosen, is theirs).
struct PlacementSearch
{
    const char *what, *candidate; // the words of the log lines
    // Where the chosen pair goes, and which pair the candidates are.  The object's own scratch: every candidate stands in as the
    // scratch while copies of a caller's side are sorted.  Other arrays: every candidate is sorted itself, against the scratch in place.
    Scratch *keys, *vals;
    size_t kbytes, vbytes; // (what the two arrays are allocated with)
    size_t count, key_size; // the calibration sort
    const char* list; // GLU_HIP_SCRATCH_TUNE_LIST, or nullptr: it does not apply
};
struct Placement
{
    bool found = false;           // a pair was chosen and is in place; else the arrays are empty
    bool short_of_memory = false; // no search: free_mib < want_mib
    size_t free_mib = 0, want_mib = 0;
    uint32_t spacer_mib = 0, tried = 0;
    double ms = 0, worst_ms = 0;
};

// The search: allocate keys, a spacer and values, free the spacer, fill, sort three times and time two of them, keep the fastest
// pair.  Leaves profiling, tuning and last_planned as a caller's sort expects them on every way out, and the best pair so far (if
// any) in place even when it fails.
glu_status search_placement(glu_radix_sort_s* s, const PlacementSearch& how, Placement& out)
{
    out = Placement();
    const bool own_scratch = how.keys == &s->keys;
    const size_t kbytes = how.kbytes, vbytes = how.vbytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GLU_OK;
    // up to 16 candidates, the value array behind spacers of 0, 0.5 .. 7.5 GiB (which spacer wins differs from process to
    // process: 24 candidates on two devices showed no period, about one in four is fast).  The search ends as soon as one
    // candidate of at least eight is 7 % faster than the slowest seen -- the speeds are discrete, fast and slow lie 5-8 %
    // apart, and the fast ones differ among themselves by 2-3 %; eight candidates take 0.13 s -- or after a second: on some devices no placement out of 32 is
    // fast, and spacers of many GiB take a quarter of a second each to allocate and free (7.9 s for 32 candidates up to
    // 15.5 GiB).  GLU_HIP_SCRATCH_TUNE_LIST=step_mib:count[:first_mib] fixes the list (no early end).
    size_t step_mib = 512, candidates = 16, first_mib = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    const bool fixed_list = how.list != nullptr;
    if (how.list) sscanf(how.list, "%zu:%zu:%zu", &step_mib, &candidates, &first_mib);
    std::vector<size_t> spacers_mib;
    for (size_t i = 0; i < std::max<size_t>(candidates, 1); i++) spacers_mib.push_back(first_mib + i * step_mib);
    // room for one candidate with its spacer and the best so far, and for the caller-side copies (twice over, to be safe)
    const size_t need_b = 2 * ((own_scratch ? 2 : 1) * (kbytes + vbytes) + (spacers_mib.back() << 20)) + ((size_t) 1 << 30);
    if (free_b < need_b)
    {
        out.short_of_memory = true, out.free_mib = free_b >> 20, out.want_mib = need_b >> 20;
        return GLU_OK;
    }
    // the calibration sorts run on the library queue and rewrite this object's tables: nothing of the caller's may still be
    // using them on another stream
    if (hipDeviceSynchronize() != hipSuccess) return fail(GLU_ERROR_DEVICE, "hipDeviceSynchronize failed before the %s placement", how.what);
    hipStream_t st = g_dev.queue;
    void *a = nullptr, *b = nullptr; // (own_scratch) the caller's side of the calibration sorts
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Cand { void* k = nullptr; void* v = nullptr; double ms = 1e30; uint32_t spacer = 0; } best;
    double worst = 0;
    uint32_t tried = 0;
    s->tuning = true; // (the sorts below must not start a search of their own)
    const int was_profiling = s->profiling;
    s->profiling = 0; // the calibration sorts are not the caller's
    how.keys->release();
    how.vals->release();
    auto done = [&](glu_status status) {
        s->profiling = was_profiling;
        (void) hipStreamSynchronize(st);
        if (a) (void) hipFree(a);
        if (b) (void) hipFree(b);
        if (e0) (void) hipEventDestroy(e0);
        if (e1) (void) hipEventDestroy(e1);
        how.keys->ptr = best.k, how.keys->size = best.k ? kbytes : 0;
        how.vals->ptr = best.v, how.vals->size = best.v ? vbytes : 0;
        s->tuning = false;
        s->last_planned = false; // glu_radix_sort_read_plan: the calibration sorts were not the caller's
        if (best.k) out.found = true, out.spacer_mib = best.spacer, out.tried = tried, out.ms = best.ms, out.worst_ms = worst;
        return status;
    };
    hipError_t err = own_scratch ? hipMalloc(&a, kbytes) : hipSuccess;
    if (err == hipSuccess && own_scratch) err = hipMalloc(&b, vbytes);
    if (err == hipSuccess) err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    if (err != hipSuccess) return done(fail(GLU_ERROR_DEVICE, "the %s placement could not start: %s", how.what, hipGetErrorString(err)));
    for (size_t spacer_mib : spacers_mib)
    {
        void *k = nullptr, *sp = nullptr, *v = nullptr;
        const bool got = hipMalloc(&k, kbytes) == hipSuccess && (!spacer_mib || hipMalloc(&sp, spacer_mib << 20) == hipSuccess) &&
                         hipMalloc(&v, vbytes) == hipSuccess;
        if (sp) (void) hipFree(sp); // the arrays stay where they are
        if (!got)
        {
            (void) hipGetLastError();
            if (!k) break; // out of memory: the best so far (or the caller's plain allocation, which reports the failure)
            (void) hipFree(k); // (no room for this spacer or for the values behind it: the next one)
            continue;
        }
        if (own_scratch) s->keys.ptr = k, s->keys.size = kbytes, s->vals.ptr = v, s->vals.size = vbytes;
        void* const sort_k = own_scratch ? a : k;
        void* const sort_v = own_scratch ? b : v;
        double ms = 1e30;
        glu_status status = GLU_OK;
        for (int rep = 0; rep < 3 && status == GLU_OK; rep++) // the first run is a warm-up
        {
            hipLaunchKernelGGL(tune_fill_kernel, dim3(g_dev.num_cus * 8), dim3(256), 0, st, (uint32_t*) sort_k, kbytes / 4, 0x5EEDu + rep);
            hipLaunchKernelGGL(tune_fill_kernel, dim3(g_dev.num_cus * 8), dim3(256), 0, st, (uint32_t*) sort_v, vbytes / 4, 77u);
            (void) hipEventRecord(e0, st);
            status = how.key_size == 8 ? sort_run<uint64_t>(s, (uint64_t*) sort_k, (uint32_t*) sort_v, how.count, 0, st)
                                       : sort_run<uint32_t>(s, (uint32_t*) sort_k, (uint32_t*) sort_v, how.count, 0, st);
            (void) hipEventRecord(e1, st);
            if (status == GLU_OK && hipEventSynchronize(e1) == hipSuccess && rep > 0)
            {
                float t = 0;
                if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms = std::min(ms, (double) t);
            }
        }
        if (own_scratch) s->keys.ptr = nullptr, s->keys.size = 0, s->vals.ptr = nullptr, s->vals.size = 0;
        (void) hipStreamSynchronize(st);
        if (status != GLU_OK)
        {
            (void) hipFree(k);
            (void) hipFree(v);
            return done(status);
        }
        if (ms < 1e29) worst = std::max(worst, ms);
        if (glu_verbose()) fprintf(stderr, "[glu_hip]   %s: keys %p values %p (spacer %zu MiB): %.3f ms\n", how.candidate, k, v, spacer_mib, ms);
        if (ms < best.ms)
        {
            if (best.k) (void) hipFree(best.k);
            if (best.v) (void) hipFree(best.v);
            best.k = k, best.v = v, best.ms = ms, best.spacer = (uint32_t) spacer_mib;
        }
        else
        {
            (void) hipFree(k);
            (void) hipFree(v);
        }
        tried++;
        if (!fixed_list && tried >= 8 && best.ms <= 0.93 * worst) break;
        if (!fixed_list && std::chrono::steady_clock::now() - t_begin > std::chrono::milliseconds(1000)) break;
    }
    return done(GLU_OK);
}
} // namespace

// The object's own scratch (sort_prepare).  Nothing chosen: sort_prepare's plain allocation follows, and reports zero candidates.
glu_status glu_hip::host::tune_scratch_placement(glu_radix_sort_s* s, size_t count, size_t key_size)
{
    // (grow-only: an array that is already larger than this count needs keeps its size)
    const PlacementSearch how{"scratch", "candidate", &s->keys, &s->vals, std::max(count * key_size, s->keys.size),
                              std::max(count * sizeof(uint32_t), s->vals.size), count, key_size, glu_env("GLU_HIP_SCRATCH_TUNE_LIST")};
    Placement p;
    GLU_TRY(search_placement(s, how, p));
    s->tuned_spacer_mib = p.spacer_mib, s->tuned_candidates = p.tried, s->tuned_ms = p.ms, s->tuned_worst_ms = p.worst_ms;
    if (glu_verbose() && p.short_of_memory)
        fprintf(stderr, "[glu_hip] scratch placement skipped: %zu MiB free, the search wants %zu MiB; plain allocation\n", p.free_mib, p.want_mib);
    if (glu_verbose() && p.found)
        fprintf(stderr, "[glu_hip] scratch placement: value array behind a %u MiB spacer, calibration sort %.3f ms (slowest candidate %.3f ms)\n",
                p.spacer_mib, p.ms, p.worst_ms);
    return GLU_OK;
}

// A PAIR of arrays for the caller's side of a sort, placed by measurement against a sorter whose own scratch is in place:
// the same search as tune_scratch_placement with the roles turned round -- the candidates (keys, values; the value array
// behind spacers of 0, 0.5 ... 7.5 GiB) are the arrays that are sorted, the sorter's scratch is what it is.  A pair of arrays
// is fast or slow whatever it is paired with, so a pair that sorts fast here is a good source and a good
// destination of any pass.  glu_dist_prepare places the sharded sort's send-side and receive-side arrays with it: of the four
// scatter passes of a rank's sort only the first one's source, the caller's slice, is then left to luck.  `keys` / `vals` are
// (re)allocated: `count` 4-byte elements each.  Explicit prepare calls only; silently the plain allocation when the search is
// switched off, the arrays are small or memory is short.
glu_status glu_hip::host::place_pair_by_measurement(glu_radix_sort_s* s, size_t count, Scratch& keys, Scratch& vals)
{
    const size_t bytes = count * sizeof(uint32_t);
    if (keys.size >= bytes && vals.size >= bytes) return GLU_OK;
    Placement p;
    if (s->tune_scratch && bytes >= kTuneMinKeyBytes && s->keys.size >= bytes && s->vals.size >= bytes)
    {
        GLU_TRY(search_placement(s, PlacementSearch{"pair", "pair candidate", &keys, &vals, bytes, bytes, count, sizeof(uint32_t), nullptr}, p));
        if (glu_verbose() && p.short_of_memory) fprintf(stderr, "[glu_hip] pair placement skipped: %zu MiB free; plain allocation\n", p.free_mib);
        if (glu_verbose() && p.found)
            fprintf(stderr, "[glu_hip] pair placement: %u candidates, calibration sort %.3f ms (slowest %.3f ms)\n", p.tried, p.ms, p.worst_ms);
    }
    if (p.found) return GLU_OK;
    GLU_TRY(keys.reserve(bytes));
    return vals.reserve(bytes);
}
