// reduce_batch_kernels.hpp -- gfx950 kernels of the BATCHED reduce (glu_reduce_run_batch_ptr / _batch_offsets_ptr): every segment of
// an array folded on its own, out[s] = op over the segment, the input left alone.  Not in the reference, whose Reduce folds one
// array per call into its element 0 (glu/Reduce.hpp:111-135).
//
// Three size classes (reduce_batch_plan is the one place that draws the lines, in BYTES of a segment):
//   short   reduce_batch_wave_kernel    up to 4 KiB: a group of 4 / 16 / 64 lanes of a wave folds one segment (up to 16, up to 64,
//                                       more elements), so a wave holds 16 / 4 / 1 segments and no lane idles on 32-element
//                                       segments.  Scalar loads, four in flight per lane, shuffles inside the group, no LDS, no
//                                       barrier, one store per segment.
//   medium  reduce_batch_block_kernel   up to 256 KiB: a workgroup folds one segment with 16-byte loads from the segment's first
//                                       16-byte-aligned element, the few elements before and behind it one per lane.
//   long    reduce_batch_chunk_kernel   the segment is cut into chunks of 256 KiB, a workgroup folds one chunk into
//                                       partials[its slot]; reduce_batch_block_kernel in COMBINE mode then folds every long
//                                       segment's partials, which lie side by side in chunk order.
// reduce_batch_bin_kernel in front (device offsets only) writes the identity of empty segments and the lists: three short lists,
// the medium list, the long list and the list of chunks.  The lists, their layout and the clamps are batch_lists.hpp's: a segment
// is [offsets[s], offsets[s + 1]), and one whose end lies below its begin or beyond `total` is EMPTY to every kernel here
// (batch_offsets_segment), so nothing outside [0, total) is ever read.
//
// Order of combination: a lane folds its elements in ascending order, groups / waves / workgroups combine in lane, wave and chunk
// order.  Which element goes to which lane depends on the segment's address (the 16-byte alignment), its length and nothing else:
// no atomics on values, nothing in arrival order.  List positions and chunk slots ARE handed out in arrival order (device
// offsets), and with equal partitions a run of slots starts at partition * chunks; every item writes a slot of its own, the slots
// of one segment are adjacent and in chunk order, and the one range whose address follows from a slot -- a long segment's run of
// partials -- is laid out from its own first element, not from a 16-byte boundary (FROM_FIRST below): partials [i * VEC,
// (i + 1) * VEC) go to lane i mod 256 for every whole pack of VEC = 16 bytes / element size, the fewer than VEC behind the last
// whole pack one to a lane from lane 0 on, wherever the run lies.  A run on a 16-byte boundary (every call with one long
// segment) is folded as it was when packs were counted from the boundary.  No identity is needed inside the folds (the `has`
// flags of block_reduce).
#pragma once

#include "batch_lists.hpp"
#include "scan_reduce_kernels.hpp"

namespace glu_hip
{
constexpr uint32_t kRbWaveBytes = 4096;         // longest segment of the short class
constexpr uint32_t kRbBlockBytes = 256 * 1024;  // longest segment of the medium class
constexpr uint32_t kRbChunkBytes = 256 * 1024;  // chunk of the long class
constexpr uint32_t kRbGroup4Elems = 16;         // up to here 4 lanes fold a segment
constexpr uint32_t kRbGroup16Elems = 64;        // up to here 16 lanes, beyond it the whole wave
constexpr int kRbThreads = 256;
constexpr int kRbWaves = kRbThreads / kW;
constexpr int kRbUnroll = 4;                    // loads in flight per lane

// host only: class (0 = empty, 1 = short, 2 = medium, 3 = long) and workgroups one segment of `count` elements is spread over
inline void reduce_batch_plan(uint64_t count, uint32_t elem_bytes, uint32_t& path, uint32_t& workgroups)
{
    workgroups = count ? 1u : 0u;
    if (count == 0) path = 0;
    else if (count <= kRbWaveBytes / elem_bytes) path = 1;
    else if (count <= kRbBlockBytes / elem_bytes) path = 2;
    else
    {
        path = 3;
        const uint64_t chunk = kRbChunkBytes / elem_bytes;
        const uint64_t n = (count + chunk - 1) / chunk;
        workgroups = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) n;
    }
}

// what the kernels that walk the six lists (the reduce's and the scan's) are told about a call
struct BatchListsArgs
{
    const uint32_t* offsets; // device offsets, or NULL: equal partitions of `count` elements
    uint64_t count;
    uint32_t total;          // device offsets: elements of the array
    uint32_t nsegs;          // segments / partitions
    uint32_t chunks_per;     // equal partitions of the long class: chunks of one partition
    int sub;                 // equal partitions of the short class: which group size (BATCH_LIST_SHORT*)
    const uint32_t* counts;  // device offsets: the list counts and the lists
    const uint32_t* lists;
    BatchListsLayout layout;
};

struct ReduceBatchIdentity
{
    uint32_t w[8]; // the operator's identity element, as the words of one element
};

// Element range of segment `seg` (see the head of the file for malformed offsets).
__device__ __forceinline__ void batch_lists_segment(const BatchListsArgs& a, uint32_t seg, uint64_t& begin, uint64_t& len)
{
    if (a.offsets) batch_offsets_segment(a.offsets, a.total, seg, begin, len);
    else
    {
        begin = (uint64_t) seg * a.count;
        len = a.count;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Binning (device offsets; `static`, as `inline` is ignored on a kernel: the batched scan's translation unit includes this header too and bins with the same kernel,
// elem_words = 0 and no `out`).  Empty segments get the identity here; every other segment is appended to the list of its class
// (wave-aggregated: one atomic per wave and list), a long one also with one entry per chunk, written by the whole wave.
// ---------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void reduce_batch_bin_kernel(BatchListsArgs a, uint32_t* __restrict__ counts, uint32_t* __restrict__ lists,
                                                               uint32_t* __restrict__ out, uint32_t elem_words, ReduceBatchIdentity identity)
{
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256u; base < a.nsegs; base += gridDim.x * 256u)
    {
        const uint32_t seg = base + threadIdx.x;
        int cls = -1;
        uint32_t nchunks = 0;
        if (seg < a.nsegs)
        {
            uint64_t begin, len;
            batch_lists_segment(a, seg, begin, len);
            if (len == 0)
            {
                for (uint32_t w = 0; w < elem_words; w++) out[(size_t) seg * elem_words + w] = identity.w[w];
            }
            else
            {
                cls = BATCH_LIST_LONG;
#pragma unroll
                for (int c = BATCH_LIST_BLOCK; c >= 0; c--)
                    if (len <= a.layout.limit[c]) cls = c;
                if (cls == BATCH_LIST_LONG) nchunks = (uint32_t) ((len + a.layout.chunk - 1) / a.layout.chunk);
            }
        }
        batch_append<BATCH_LIST_LONG>(cls, seg, lane, a.layout, counts, lists);
        // Long segments are few (each is longer than a chunk): atomics of its own for each.  First its run of chunk slots; its
        // place in the long list only if the whole run lies inside the chunk list, so that every listed segment has all its
        // partials.  (Non-decreasing offsets always fit; of overlapping segments those that do not get no result.)
        uint32_t slot = a.layout.capacity[BATCH_LIST_CHUNKS];
        if (cls == BATCH_LIST_LONG)
        {
            const unsigned long long got = atomicAdd(reinterpret_cast<unsigned long long*>(counts + kBatchCountChunks), (unsigned long long) nchunks);
            if (got < a.layout.capacity[BATCH_LIST_CHUNKS]) slot = (uint32_t) got;
            if (got + nchunks <= a.layout.capacity[BATCH_LIST_CHUNKS])
            {
                const uint32_t at = atomicAdd(&counts[kBatchCountLong], 1u);
                if (at < a.layout.capacity[BATCH_LIST_LONG])
                {
                    uint2* entry = reinterpret_cast<uint2*>(lists + a.layout.start[BATCH_LIST_LONG]) + at;
                    *entry = make_uint2(seg, slot);
                }
            }
        }
        // every slot below the chunk list's length gets its entry, also from a run that only begins inside the list
        uint64_t m = __ballot(cls == BATCH_LIST_LONG);
        while (m) // wave-uniform
        {
            const int src = __ffsll((unsigned long long) m) - 1;
            m &= m - 1;
            const uint32_t s_seg = (uint32_t) __shfl((int) seg, src);
            const uint32_t s_slot = (uint32_t) __shfl((int) slot, src);
            const uint32_t s_n = (uint32_t) __shfl((int) nchunks, src);
            uint2* chunks = reinterpret_cast<uint2*>(lists + a.layout.start[BATCH_LIST_CHUNKS]);
            for (uint32_t c = lane; c < s_n; c += kW)
                if ((uint64_t) s_slot + c < a.layout.capacity[BATCH_LIST_CHUNKS]) chunks[s_slot + c] = make_uint2(s_seg, c);
        }
    }
}

// out[s] = identity for s < n (equal partitions of no elements)
static __global__ __launch_bounds__(256) void reduce_batch_fill_kernel(uint32_t* __restrict__ out, uint32_t n, uint32_t elem_words,
                                                                ReduceBatchIdentity identity)
{
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n; s += gridDim.x * 256u)
        for (uint32_t w = 0; w < elem_words; w++) out[(size_t) s * elem_words + w] = identity.w[w];
}

// ---------------------------------------------------------------------------------------------------------
// Short segments: a group of 1 << lg lanes per segment.
// ---------------------------------------------------------------------------------------------------------
template<int OP, typename S, int N>
__global__ __launch_bounds__(kRbThreads) void reduce_batch_wave_kernel(const Elem<S, N>* __restrict__ data, Elem<S, N>* __restrict__ out,
                                                                        BatchListsArgs a)
{
    using T = Elem<S, N>;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // device offsets: a third of the grid walks each short list; equal partitions: the whole grid, the one group size of `count`
    const int sub = a.lists ? (int) (blockIdx.x % 3u) : a.sub;
    const uint32_t block = a.lists ? blockIdx.x / 3u : blockIdx.x;
    const uint32_t blocks = a.lists ? gridDim.x / 3u : gridDim.x;
    const uint32_t lg = sub == BATCH_LIST_SHORT4 ? 2u : sub == BATCH_LIST_SHORT16 ? 4u : 6u;
    const uint32_t G = 1u << lg, per_wave = kW >> lg;
    const uint32_t n = a.lists ? batch_list_length(a.counts, a.layout, sub) : a.nsegs;
    const uint32_t* list = a.lists ? a.lists + a.layout.start[sub] : nullptr;
    const uint32_t j = lane & (G - 1u);

    for (uint64_t first = (uint64_t) (block * kRbWaves + wave) * per_wave; first < n; first += (uint64_t) blocks * kRbWaves * per_wave)
    {
        const uint64_t li = first + (lane >> lg);
        uint32_t seg = 0;
        uint64_t begin = 0, len = 0;
        if (li < n)
        {
            seg = list ? list[li] : (uint32_t) li;
            batch_lists_segment(a, seg, begin, len);
        }
        const T* p = data + begin;
        T acc = zero_elem<S, N>();
        bool has = false;
        for (uint32_t i = j; i < (uint32_t) len; i += kRbUnroll * G)
        {
            T v[kRbUnroll];
#pragma unroll
            for (int u = 0; u < kRbUnroll; u++)
                if (i + u * G < (uint32_t) len) v[u] = load_streaming(&p[i + u * G]);
#pragma unroll
            for (int u = 0; u < kRbUnroll; u++)
                if (i + u * G < (uint32_t) len)
                {
                    acc = has ? combine<OP>(acc, v[u]) : v[u];
                    has = true;
                }
        }
#pragma unroll
        for (uint32_t off = 32; off > 0; off >>= 1)
        {
            if (off >= G) continue; // wave-uniform
            T o = shfl_down_t(acc, (int) off);
            const int oh = __shfl_down((int) has, (int) off, kW);
            const bool other_ok = (j + off < G) && oh;
            if (other_ok) acc = has ? combine<OP>(acc, o) : o;
            has = has || other_ok;
        }
        if (j == 0 && has) out[seg] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The fold of one contiguous range by a workgroup's threads: elements before the first 16-byte boundary and behind the last whole
// 16-byte pack go one to a lane, the packs in between are read with 16-byte non-temporal loads, kRbUnroll in flight per lane.
// FROM_FIRST (the partials of a long segment, whose slot -- and with it the run's alignment -- depends on the order in which
// segments were binned): the packs are counted from the range's own first element instead, so that which element goes to which
// lane depends on the range's length alone; a pack is then read 16 bytes at a time only if the range happens to be aligned,
// element by element otherwise, into the same lane and in the same order.
// ---------------------------------------------------------------------------------------------------------
template<int OP, typename S, int N, bool FROM_FIRST = false>
__device__ __forceinline__ void reduce_batch_fold_range(const Elem<S, N>* __restrict__ p, uint32_t len, uint32_t tid, Elem<S, N>& acc, bool& has)
{
    using T = Elem<S, N>;
    constexpr uint32_t VEC = sizeof(T) < 16 ? 16 / (uint32_t) sizeof(T) : 1;
    using P = Pack<T, (int) VEC>;
    auto fold = [&](const T& v) {
        acc = has ? combine<OP>(acc, v) : v;
        has = true;
    };
    uint32_t head = 0;
    if (VEC > 1 && !FROM_FIRST)
    {
        head = (uint32_t) (((16u - (uint32_t) ((uintptr_t) p & 15u)) & 15u) / sizeof(T));
        if (head > len) head = len;
        if (tid < head) fold(p[tid]);
    }
    const bool aligned = !FROM_FIRST || ((uintptr_t) p & 15u) == 0; // 16-byte loads are possible (workgroup-uniform)
    const P* packs = reinterpret_cast<const P*>(p + head);
    auto load_pack = [&](uint32_t i) -> P {
        if (aligned) return load_streaming(&packs[i]);
        P v;
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++) v.v[k] = p[i * VEC + k]; // (FROM_FIRST: head == 0)
        return v;
    };
    const uint32_t npacks = (len - head) / VEC;
    uint32_t i = tid;
    for (; i + (kRbUnroll - 1) * kRbThreads < npacks; i += kRbUnroll * kRbThreads)
    {
        P v[kRbUnroll];
#pragma unroll
        for (int u = 0; u < kRbUnroll; u++) v[u] = load_pack(i + u * kRbThreads);
#pragma unroll
        for (int u = 0; u < kRbUnroll; u++)
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++) fold(v[u].v[k]);
    }
    for (; i < npacks; i += kRbThreads)
    {
        const P v = load_pack(i);
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++) fold(v.v[k]);
    }
    if (VEC > 1)
    {
        const uint32_t t = head + npacks * VEC + tid; // < VEC elements behind the last pack
        if (t < len) fold(p[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Medium segments (combine == 0): src = the caller's array, one workgroup per entry of the medium list (or per partition).
// Long segments' second step (combine == 1): src = the partials, one workgroup per entry of the long list (or per partition) folds
// the segment's run of partials, laid out from the run's first element.
// ---------------------------------------------------------------------------------------------------------
template<int OP, typename S, int N>
__global__ __launch_bounds__(kRbThreads) void reduce_batch_block_kernel(const Elem<S, N>* __restrict__ src, Elem<S, N>* __restrict__ out,
                                                                         BatchListsArgs a, int combine_partials)
{
    using T = Elem<S, N>;
    __shared__ T wtmp[kRbWaves];
    __shared__ uint32_t whas[kRbWaves];
    const uint32_t tid = threadIdx.x;
    const int c = combine_partials ? BATCH_LIST_LONG : BATCH_LIST_BLOCK;
    const uint32_t n = a.lists ? batch_list_length(a.counts, a.layout, c) : a.nsegs;
    for (uint32_t li = blockIdx.x; li < n; li += gridDim.x)
    {
        uint32_t seg = li;
        uint64_t begin, len;
        if (!combine_partials)
        {
            if (a.lists) seg = a.lists[a.layout.start[BATCH_LIST_BLOCK] + li];
            batch_lists_segment(a, seg, begin, len);
        }
        else if (a.lists)
        {
            const uint2 entry = reinterpret_cast<const uint2*>(a.lists + a.layout.start[BATCH_LIST_LONG])[li];
            seg = entry.x;
            begin = entry.y;
            uint64_t sb, sl;
            batch_lists_segment(a, seg, sb, sl);
            len = (sl + a.layout.chunk - 1) / a.layout.chunk; // (a listed segment's whole run lies inside the chunk list)
        }
        else
        {
            begin = (uint64_t) li * a.chunks_per;
            len = a.chunks_per;
        }
        T acc = zero_elem<S, N>();
        bool has = false;
        // (workgroup-uniform; elements of 16 bytes or more have no packs to count from anywhere)
        if (sizeof(T) < 16 && combine_partials) reduce_batch_fold_range<OP, S, N, true>(src + begin, (uint32_t) len, tid, acc, has);
        else reduce_batch_fold_range<OP>(src + begin, (uint32_t) len, tid, acc, has);
        bool rh;
        const T r = block_reduce<OP>(acc, has, wtmp, whas, tid, rh);
        if (tid == 0 && rh) out[seg] = r;
        __syncthreads(); // wtmp / whas are read by every thread above and written again in the next round
    }
}

// Long segments' first step: partials[slot] = fold of one chunk, one workgroup per entry of the chunk list (device offsets) or
// per (partition, chunk) pair.
template<int OP, typename S, int N>
__global__ __launch_bounds__(kRbThreads) void reduce_batch_chunk_kernel(const Elem<S, N>* __restrict__ data, Elem<S, N>* __restrict__ partials,
                                                                         BatchListsArgs a, uint64_t nitems)
{
    using T = Elem<S, N>;
    __shared__ T wtmp[kRbWaves];
    __shared__ uint32_t whas[kRbWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.lists ? (uint64_t) batch_list_length(a.counts, a.layout, BATCH_LIST_CHUNKS) : nitems;
    for (uint64_t slot = blockIdx.x; slot < n; slot += gridDim.x)
    {
        uint32_t seg, chunk;
        if (a.lists)
        {
            const uint2 entry = reinterpret_cast<const uint2*>(a.lists + a.layout.start[BATCH_LIST_CHUNKS])[slot];
            seg = entry.x;
            chunk = entry.y;
        }
        else
        {
            seg = (uint32_t) (slot / a.chunks_per);
            chunk = (uint32_t) (slot % a.chunks_per);
        }
        uint64_t begin, len;
        batch_lists_segment(a, seg, begin, len);
        const uint64_t at = (uint64_t) chunk * a.layout.chunk;
        T acc = zero_elem<S, N>();
        bool has = false;
        if (at < len) // (workgroup-uniform)
        {
            const uint64_t left = len - at;
            reduce_batch_fold_range<OP>(data + begin + at, left < a.layout.chunk ? (uint32_t) left : a.layout.chunk, tid, acc, has);
        }
        bool rh;
        const T r = block_reduce<OP>(acc, has, wtmp, whas, tid, rh);
        if (tid == 0 && rh) partials[slot] = r;
        __syncthreads();
    }
}

} // namespace glu_hip
