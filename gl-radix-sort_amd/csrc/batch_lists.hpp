// batch_lists.hpp -- the segment lists of the batched operators (radix_batch_kernels.hpp, reduce_batch_kernels.hpp,
// scan_batch_kernels.hpp): a binning kernel appends every segment of a call with device offsets to the list of its length class,
// one kernel per class then walks its list.  What decides which memory a segment and a list may touch, once for the three: the
// layout of the lists (plain C++: tests/test_batch_lists_layout.py includes this header with a host compiler), the two clamps, the append.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>

namespace glu_hip
{
// Lists 0 .. 3 hold the segments of the four bounded classes, shortest class first, one word (the segment's index) per entry: the
// sort's wave class and its three workgroup tiles; the reduce's and the scan's groups of 4 / 16 / 64 lanes and their workgroup class.
enum
{
    BATCH_LIST_SHORT4 = 0,
    BATCH_LIST_SHORT16 = 1,
    BATCH_LIST_SHORT64 = 2,
    BATCH_LIST_BLOCK = 3,
    BATCH_LIST_LONG = 4,   // every longer segment.  Wide form (reduce, scan), uint2 entries: segment, slot of its first chunk
    BATCH_LIST_CHUNKS = 5, // wide form only, uint2 entries: segment, chunk of the segment
    BATCH_LISTS = 6
};
// The count line in front of the lists.  counts[0 .. 3]: lengths of the bounded lists; counts[4 .. 5]: chunk slots handed out, ONE
// 64-bit counter (overlapping long segments -- malformed offsets only -- can ask for far more than 2^32 of them, and it must not
// wrap); counts[6]: length of the long list.
constexpr int kBatchCountChunks = 4, kBatchCountLong = 6, kBatchCounts = 7;
constexpr int batch_count_word(int list) { return list == BATCH_LIST_LONG ? kBatchCountLong : list; }

struct BatchListsLayout
{
    uint32_t start[BATCH_LISTS];    // first word of list c in `lists` (which lie behind the counts, not over them)
    uint32_t capacity[BATCH_LISTS]; // entries list c holds
    uint32_t limit[4];              // longest segment (elements) of the four bounded classes; longer ones are long
    uint32_t chunk;                 // elements of a chunk (0: no chunk list)
};

// What an operator says about its classes.
struct BatchClasses
{
    uint32_t shortest; // shortest segment that is listed at all (elements): shorter ones are in no list
    uint32_t limit[4]; // BatchListsLayout::limit
    uint32_t chunk;    // BatchListsLayout::chunk
    bool wide;         // the long list and the chunk list have 8-byte entries (else: 4-byte entries and no chunk list)
};

// The lists of a batch of `num_segments` segments inside `total` elements; `words`: what they take together.  List c holds
// min(num_segments, total / shortest length of its class) entries, as many segments of its class as fit `total`: non-decreasing
// offsets cannot overflow it.  The lists lie back to back, an 8-byte list from an even word on.  The chunk list holds a chunk per
// whole chunk of `total` and one more per long segment (its last, partial one), and nothing when the long list holds nothing.
// (No long segment can exist then: it has more than limit[BATCH_LIST_BLOCK] elements, and an array and a batch that hold one give
// the long list min(num_segments, total / (limit[BATCH_LIST_BLOCK] + 1)) >= 1 entries.)
inline BatchListsLayout batch_lists_layout(const BatchClasses& cls, size_t total, size_t num_segments, size_t& words)
{
    BatchListsLayout l = {};
    l.chunk = cls.chunk;
    for (int c = 0; c < BATCH_LIST_LONG; c++) l.limit[c] = cls.limit[c];
    size_t at = 0;
    for (int c = 0; c <= BATCH_LIST_LONG; c++)
    {
        const size_t entry_words = c == BATCH_LIST_LONG && cls.wide ? 2 : 1;
        const size_t fit = total / (c == 0 ? (size_t) cls.shortest : (size_t) cls.limit[c - 1] + 1);
        at = (at + entry_words - 1) & ~(entry_words - 1);
        l.start[c] = (uint32_t) at;
        l.capacity[c] = (uint32_t) (num_segments < fit ? num_segments : fit);
        at += entry_words * l.capacity[c];
    }
    l.start[BATCH_LIST_CHUNKS] = (uint32_t) at;
    if (cls.chunk && l.capacity[BATCH_LIST_LONG]) l.capacity[BATCH_LIST_CHUNKS] = (uint32_t) (total / cls.chunk + l.capacity[BATCH_LIST_LONG]);
    words = at + 2 * (size_t) l.capacity[BATCH_LIST_CHUNKS];
    return l;
}

#ifdef __HIPCC__
#define GLU_BATCH_FN __host__ __device__ __forceinline__
#else
#define GLU_BATCH_FN inline // (a host compiler: the test programs)
#endif

// The clamp of a segment, on the two offsets already loaded: [b, e) where b <= e <= total, else the empty segment at b.  Plain C++,
// so that a host program (tests/test_histogram_batch_walk.py) walks whole calls through the rule the kernels use.
template<typename I>
GLU_BATCH_FN void batch_clamp_segment(uint32_t b, uint32_t e, const uint32_t& total, I& begin, I& len)
{
    if (e < b || e > total) e = b;
    begin = b;
    len = e - b;
}

// Whether the run of `nchunks` chunk slots from `got` on lies inside a chunk list of `capacity` slots: only then is a long segment
// listed, so that every listed segment has all its chunks (the batched reduce's rule; the batched histogram's binning calls this).
GLU_BATCH_FN bool batch_chunk_run_fits(uint64_t got, uint32_t nchunks, uint32_t capacity) { return got + nchunks <= capacity; }

#ifdef __HIPCC__
// Element range of segment `seg` of device offsets, which the host cannot check: a segment that ends below its begin or beyond
// `total` is empty, so no kernel reads or writes outside [0, total) whatever the array holds.
// (begin, len: 32 bits wide in the sort, 64 in the reduce and the scan.  `total` by reference: a caller that keeps it in a struct of
// kernel arguments has it read where it is compared, and compiles to what it did with the clamp written out in place.)
template<typename I>
__device__ __forceinline__ void batch_offsets_segment(const uint32_t* offsets, const uint32_t& total, uint32_t seg, I& begin, I& len)
{
    const uint32_t b = offsets[seg];
    const uint32_t e = offsets[seg + 1];
    batch_clamp_segment(b, e, total, begin, len);
}

// How many entries of a list a kernel walks: the count the binning kernel wrote, never more than the list holds.
__device__ __forceinline__ uint32_t batch_list_length(uint64_t count, uint32_t capacity) { return count < capacity ? (uint32_t) count : capacity; }

// ... of list c behind the count line `counts`
__device__ __forceinline__ uint32_t batch_list_length(const uint32_t* counts, const BatchListsLayout& layout, int c)
{
    const uint64_t n = c == BATCH_LIST_CHUNKS ? *reinterpret_cast<const unsigned long long*>(counts + kBatchCountChunks)
                                              : (uint64_t) counts[batch_count_word(c)];
    return n < layout.capacity[c] ? (uint32_t) n : layout.capacity[c];
}

// Binning: every lane of a wave comes here with its segment `seg` and the segment's class `cls` (-1: none); the segments of the
// one-word lists 0 .. LISTS - 1 are appended to them.  Wave-aggregated: one vector atomic per wave and class, the lanes ranked
// behind it with v_mbcnt.  Order inside a list does not matter.
template<int LISTS>
__device__ __forceinline__ void batch_append(int cls, uint32_t seg, uint32_t lane, const BatchListsLayout& layout,
                                             uint32_t* __restrict__ counts, uint32_t* __restrict__ lists)
{
#pragma unroll
    for (int c = 0; c < LISTS; c++)
    {
        const uint64_t m = __ballot(cls == c);
        if (m == 0) continue; // wave-uniform
        const int leader = __ffsll((unsigned long long) m) - 1;
        uint32_t first = 0;
        if ((int) lane == leader) first = atomicAdd(&counts[batch_count_word(c)], (uint32_t) __popcll(m));
        first = (uint32_t) __shfl((int) first, leader);
        if (cls == c)
        {
            const uint32_t at = first + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
            if (at < layout.capacity[c]) lists[layout.start[c] + at] = seg; // (cannot overflow with non-decreasing offsets)
        }
    }
}

// Binning, the long class of the wide form: every lane of a wave comes here, `is_long` where its segment `seg` is longer than the
// workgroup class and has `nchunks` chunks.  What reduce_batch_bin_kernel spells out in place, for kernels that bin by themselves
// (the batched histogram's): a long segment takes its run of chunk slots with one 64-bit atomic and its place in the long list only
// if the whole run lies inside the chunk list (batch_chunk_run_fits); every slot below the chunk list's capacity gets its entry,
// written by the whole wave.  Non-decreasing offsets always fit; of overlapping segments those that do not get no result.
__device__ __forceinline__ void batch_append_long(bool is_long, uint32_t seg, uint32_t nchunks, uint32_t lane, const BatchListsLayout& layout,
                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ lists)
{
    const uint32_t capacity = layout.capacity[BATCH_LIST_CHUNKS];
    uint32_t slot = capacity;
    if (is_long)
    {
        const unsigned long long got = atomicAdd(reinterpret_cast<unsigned long long*>(counts + kBatchCountChunks), (unsigned long long) nchunks);
        if (got < capacity) slot = (uint32_t) got;
        if (batch_chunk_run_fits(got, nchunks, capacity))
        {
            const uint32_t at = atomicAdd(&counts[kBatchCountLong], 1u);
            if (at < layout.capacity[BATCH_LIST_LONG]) reinterpret_cast<uint2*>(lists + layout.start[BATCH_LIST_LONG])[at] = make_uint2(seg, slot);
        }
    }
    uint64_t m = __ballot(is_long);
    while (m) // wave-uniform
    {
        const int src = __ffsll((unsigned long long) m) - 1;
        m &= m - 1;
        const uint32_t s_seg = (uint32_t) __shfl((int) seg, src);
        const uint32_t s_slot = (uint32_t) __shfl((int) slot, src);
        const uint32_t s_n = (uint32_t) __shfl((int) nchunks, src);
        uint2* chunks = reinterpret_cast<uint2*>(lists + layout.start[BATCH_LIST_CHUNKS]);
        for (uint32_t c = lane; c < s_n; c += 64u)
            if ((uint64_t) s_slot + c < capacity) chunks[s_slot + c] = make_uint2(s_seg, c);
    }
}
#endif // __HIPCC__

} // namespace glu_hip
