// glu_host.hpp -- what the translation units of libglu_hip.so share on the HOST side: the error slot behind glu_last_error(), the
// one device of the process and its queue, the buffer registry behind the glu_buffer handles, grow-only scratch allocations.
// Defined in glu_core.hip.  The library is built from twenty-one translation units (it was one, a three-minute compile):
//   glu_core.hip              errors, device, buffers, timer
//   glu_hip.hip               RadixSort's whole-key driver: sort_prepare, sort_bits (what a call decides before it enqueues:
//                             sort_call_plan.hpp, plain C++), the options and the entry points that are not about segments or placement
//   glu_sort_placement.hip    the placement search: large scratch arrays placed by measurement
//   glu_sort_segments.hip     the segmented passes (long runs of a whole-key sort) and the segmented sort (its host arithmetic:
//                             seg_plan.hpp, plain C++)
//   glu_dist.hip              the sharded sort (glu_dist_*); no kernels of its own
//                             (these four and the batched sort call one another through glu_sort_driver.hpp)
//   glu_sort_passes_u32.hip   the launchers of one counting pass for 4-byte keys (glu_sort_passes.hpp over glu_sort_object.hpp)
//   glu_sort_passes_u64.hip   the same for 8-byte keys
//   glu_sort_finish.hip       the launches of the in-LDS pass (radix_lds_bucket.hpp, radix_lds_finish.hpp: a hundred kernel instantiations)
//   glu_sort_batch.hip        the batched sort: every segment of an array on its own (radix_batch_kernels.hpp)
//   glu_scan_reduce.hip       BlellochScan and Reduce
//   glu_reduce_batch.hip      the batched reduce: every segment of an array folded on its own (reduce_batch_kernels.hpp)
//   glu_scan_batch.hip        the batched scan: every segment of an array scanned on its own (scan_batch_kernels.hpp)
//   glu_key_runs.hip          key runs: the offsets of the runs of equal keys, for the three batched units (key_runs_kernels.hpp)
//   glu_select.hip            select: stable stream compaction by a stencil and a comparison (select_kernels.hpp), and its batched form (select_batch_kernels.hpp)
//   glu_sorted_search.hip     sorted search: lower and upper bounds of many needles in a sorted haystack (sorted_search_kernels.hpp),
//                             and every segment's needles in its own haystack (sorted_search_batch_kernels.hpp over search_batch_walk.hpp)
//   glu_merge.hip             merge: two sorted arrays of keys and values into one, stable (merge_kernels.hpp over merge_path.hpp)
//   glu_histogram.hip         histogram: counts per bin over even bins or sorted edges (histogram_kernels.hpp over histogram_bins.hpp),
//                             and every segment's counts in a row of its own (histogram_batch_kernels.hpp over histogram_batch_walk.hpp)
//   glu_expand.hip            expand: segment, rank and item per element from the offsets (expand_kernels.hpp over expand_path.hpp)
//   glu_gather.hip            gather and scatter: items fetched or placed by device indices (gather_kernels.hpp over gather_walk.hpp)
//   glu_top_k.hip             top-k: the k smallest or largest keys and their indices by a radix select (topk_kernels.hpp over topk_pick.hpp)
//   glu_top_k_batch.hip       batched top-k: the k best keys of every segment in one call (topk_batch_kernels.hpp over topk_batch_plan.hpp)
// The three batched units share glu_batch_host.hpp on the host side and batch_lists.hpp (the segment lists) on both sides.
// Key runs, select, sorted search, merge, histogram, expand and top-k share glu_tile_host.hpp on the host side; the first three, histogram
// and top-k share tile_span.hpp (the tiles, the packs of an array at any alignment) on both sides; histogram and top-k share the counting
// walk of histogram_walk.hpp.
// The argument rules every unit checks by (key types, limits, overlap, alignment, items, handles, out-parameters) are glu_args.hpp's,
// plain C++ that this header includes; the life of an operator object is create_object / destroy_object below, over its release().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>

#include "glu_args.hpp"

namespace glu_hip
{
namespace host
{
extern thread_local std::string g_last_error;

// GLU_VERBOSE=1: allocations and placement searches are narrated on stderr (read once per process)
bool glu_verbose();

// Every other environment variable the library reads goes through here: defaults of new sort objects (kSortOptions), the
// tuning lists of the placement search / scan / reduce, and the test hooks of glu_dist (fault injection, the RCCL test double).
const char* glu_env(const char* name);

#define HIP_TRY(expr)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? GLU_ERROR_OUT_OF_MEMORY : GLU_ERROR_DEVICE, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                                        \
    } while (0)

// ------------------------------------------------------------------------------------------------------------
// device / queue state (one device per process)
// ------------------------------------------------------------------------------------------------------------
struct Device
{
    std::mutex mutex;
    bool ready = false;
    int requested = -1;
    int id = 0;
    int num_cus = 256;
    hipStream_t queue = nullptr;
    hipDeviceProp_t props;
};
extern Device g_dev;

glu_status ensure_device();

// Every public entry point runs this first: the device is initialised once per process, and the calling thread's
// current HIP device is made the library's device (a new thread's current device is 0, and an application may switch
// devices between two library calls -- torch.cuda.device(k), hipSetDevice -- so the current device is asked for every
// time instead of being remembered per thread: without this, scratch would be allocated on one device and the kernels
// launched on a stream of another).
glu_status enter();

inline hipStream_t pick_stream(void* stream) { return stream ? (hipStream_t) stream : g_dev.queue; }

// ------------------------------------------------------------------------------------------------------------
// buffers
// ------------------------------------------------------------------------------------------------------------
struct Buffer
{
    void* ptr = nullptr;
    size_t size = 0;
    bool owned = true;
};
glu_status lookup(glu_buffer h, Buffer& out, const char* what);

// GLU_HIP_SCRATCH_FILL (a test switch, read at every growth): a new scratch allocation is filled with that byte, 0 .. 255, before
// anything can be enqueued on it, and its size is added to what glu_scratch_filled_bytes() reads.  What a fresh allocation holds is
// an input of every kernel that no caller controls; the operators may not depend on it ("Who writes scratch first").
// Unset: one getenv per growth and nothing else.  Any other value refuses the call that grows, and the object keeps no allocation.
glu_status fill_new_scratch(void* ptr, size_t bytes);

// grow-only device allocation owned by an operator object
struct Scratch
{
    void* ptr = nullptr;
    size_t size = 0;
    glu_status reserve(size_t bytes)
    {
        if (bytes <= size) return GLU_OK;
        if (ptr) HIP_TRY(hipFree(ptr));
        ptr = nullptr;
        size = 0;
        HIP_TRY(hipMalloc(&ptr, bytes));
        const glu_status filled = fill_new_scratch(ptr, bytes);
        if (filled != GLU_OK)
        {
            (void) hipFree(ptr);
            ptr = nullptr;
            return filled;
        }
        size = bytes;
        if (glu_verbose()) fprintf(stderr, "[glu_hip] scratch reallocated to: %zu\n", bytes);
        return GLU_OK;
    }
    void release()
    {
        if (ptr) (void) hipFree(ptr);
        ptr = nullptr;
        size = 0;
    }
};

// The life of an operator object T: T::release() gives back everything the object owns -- its Scratch members, and for the sort
// object (glu_sort_object.hpp) its pinned host words, events and side stream as well.  The sharded sort keeps a life cycle of its
// own (glu_dist.hip: it owns communicators).
// glu_*_create: `init` sets the new object up from the call's other arguments, or from the environment, and may refuse them.
template<typename T, typename Init>
glu_status create_object(T** out, Init&& init)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(out, "out"));
    T* object = new T();
    const glu_status status = init(*object);
    if (status != GLU_OK)
    {
        object->release();
        delete object;
        return status;
    }
    *out = object;
    return GLU_OK;
}
template<typename T>
glu_status create_object(T** out)
{
    return create_object(out, [](T&) { return GLU_OK; });
}

// glu_*_destroy: NULL is fine
template<typename T>
glu_status destroy_object(T* object)
{
    GLU_TRY(enter());
    if (!object) return GLU_OK;
    (void) hipDeviceSynchronize(); // (a caller stream may still run its kernels)
    object->release();
    delete object;
    return GLU_OK;
}
} // namespace host
} // namespace glu_hip
