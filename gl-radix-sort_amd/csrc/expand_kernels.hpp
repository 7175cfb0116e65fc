// expand_kernels.hpp -- gfx950 kernels of EXPAND (glu_expand_run_ptr): from the offsets of segments to the segment, the rank inside
// it and the segment's item for every element.  The inverse of key runs; numpy.repeat / run-length decode.  Not in the reference.
//
// For position j of [0, total): c(j) = the number of r in [0, num_segments] with offsets[r] <= j; j is covered iff
// 1 <= c(j) <= num_segments, and then out_segments[j] = s = c(j) - 1, out_ranks[j] = j - offsets[s], out_items[j] = items[s].
// Positions that are not covered are not written.
//
// The algorithm is a load-balancing search: merge path between the offsets (side A, first on ties) and the positions 0 .. total - 1
// (side B); its arithmetic is expand_path.hpp over merge_path.hpp (plain C++, tested on the host).
//   partition  expand_partition_kernel: one thread per tile boundary d = t * TILE of the MERGED sequence, t = 0 .. tiles:
//              split[t] = the offsets among its first d items (kernel-uniform trip count, every probe clamped).  Cutting the merged
//              sequence bounds a tile's offsets PLUS outputs by TILE: a long run of empty segments becomes tiles that write nothing.
//   tile       expand_tile_kernel: one workgroup of 256 per tile.  Its offsets (and the one in front of them) go to LDS; the last
//              offset of every run of equal ones stores its slot at marks[offset - b0] (plain stores, one writer per word); an
//              inclusive max-scan of the marks (ITEMS words per thread, DPP inside the wave, LDS between the four waves) leaves at
//              every position the slot of its segment's offset.  Every requested output is then written by contiguous lanes in whole
//              16-byte packs from the 16-byte boundary at or below its first element; the packs that hold the first and the last
//              output of the tile, or a position that is not covered, go element by element.
// No atomics, no look-back, nothing waits for another workgroup.  Offsets that are not sorted give unspecified contents, but the
// tile still reads only its clamped range of offsets, writes only positions of its clamped range below total, and gathers only
// items[s] with s < num_segments (expand_segment).
#pragma once

#include "expand_path.hpp"
#include "scan_reduce_kernels.hpp"

namespace glu_hip
{
struct ExpandArgs
{
    const uint32_t* offsets; // na = num_segments + 1 words
    const void* items;       // num_segments items of ITEM_WORDS words, or null
    void* out_items;
    uint32_t* out_segments;
    uint32_t* out_ranks;
    uint32_t na, nb; // num_segments + 1, total
    uint32_t tiles;  // ceil((na + nb) / TILE)
    uint32_t* split; // tiles + 1 words
};

__global__ __launch_bounds__(kExpandThreads) void expand_partition_kernel(ExpandArgs e)
{
    const uint32_t t = blockIdx.x * kExpandThreads + threadIdx.x;
    if (t > e.tiles) return;
    e.split[t] = expand_split(expand_diag(t, e.na + e.nb), e.na, e.nb, [&](uint32_t i, bool any) { return any ? e.offsets[i] : 0u; });
}

// Wave64 inclusive maximum with DPP moves (wave_exclusive_sum of radix_sort_kernels.hpp with max for +: a lane without a source
// reads 0, the identity of the maximum of unsigned words).  `before`: the maximum of the lanes in front (0 in lane 0).
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v, uint32_t& before)
{
    int m = (int) v;
    const auto mx = [](int a, int b) { return (int) ((uint32_t) a > (uint32_t) b ? (uint32_t) a : (uint32_t) b); };
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x111, 0xf, 0xf, false)); // row_shr:1
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x112, 0xf, 0xf, false)); // row_shr:2
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x114, 0xf, 0xf, false)); // row_shr:4
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x118, 0xf, 0xf, false)); // row_shr:8   -> scanned inside rows of 16
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x142, 0xa, 0xf, false)); // row_bcast:15 into rows 1 and 3
    m = mx(m, __builtin_amdgcn_update_dpp(0, m, 0x143, 0xc, 0xf, false)); // row_bcast:31 into rows 2 and 3
    before = (uint32_t) __builtin_amdgcn_update_dpp(0, m, 0x138, 0xf, 0xf, false); // wave_shr:1
    return (uint32_t) m;
}

// One output array of 4- or 8-byte elements over the tile's positions [b0, b0 + count): `out` points at element b0.  scanned[i] is
// the slot of position b0 + i; value(i, segment, slot) is its element.  Pack p counts from the 16-byte boundary at or below `out`.
template<typename T, typename Value>
__device__ __forceinline__ void expand_store_tile(const uint32_t* scanned, uint32_t a0, uint32_t num_segments, uint32_t count, T* out,
                                                  Value value)
{
    constexpr uint32_t VEC = 16 / sizeof(T);
    const uint32_t lo = (uint32_t) (((uintptr_t) out & 15u) / sizeof(T));
    T* base = out - lo;
    const uint32_t hi = lo + count, packs = (hi + VEC - 1) / VEC;
    for (uint32_t p = threadIdx.x; p < packs; p += kExpandThreads)
    {
        const uint32_t e0 = p * VEC;
        Pack<T, VEC> pack;
        bool live[VEC], whole = true;
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            const bool inside = e0 + k >= lo && e0 + k < hi;
            const uint32_t i = inside ? e0 + k - lo : 0u; // i < count
            const uint32_t slot = scanned[i];
            uint32_t segment;
            live[k] = expand_segment(a0, slot, num_segments, &segment) && inside;
            pack.v[k] = live[k] ? value(i, segment, slot) : T();
            whole = whole && live[k];
        }
        if (whole)
            *reinterpret_cast<Pack<T, VEC>*>(base + e0) = pack;
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++)
                if (live[k]) base[e0 + k] = pack.v[k];
        }
    }
}

// Items of 16 or 32 bytes (PACKS = 1 or 2 packs each): items and out_items are aligned to 16 bytes, so every pack is whole;
// contiguous lanes write contiguous packs.
template<uint32_t PACKS>
__device__ __forceinline__ void expand_store_wide(const uint32_t* scanned, uint32_t a0, uint32_t num_segments, uint32_t count,
                                                  const Pack<uint32_t, 4>* items, Pack<uint32_t, 4>* out)
{
    for (uint32_t q = threadIdx.x; q < count * PACKS; q += kExpandThreads)
    {
        const uint32_t i = q / PACKS, part = q % PACKS;
        uint32_t segment;
        if (expand_segment(a0, scanned[i], num_segments, &segment)) out[q] = items[(size_t) segment * PACKS + part];
    }
}

// ITEM_WORDS: 0 (no items), 1, 2, 4 or 8 words an item
template<uint32_t ITEM_WORDS>
__global__ __launch_bounds__(kExpandThreads) void expand_tile_kernel(ExpandArgs e)
{
    constexpr uint32_t ITEMS = kExpandItems, TILE = kExpandTile, WAVES = kExpandThreads / 64;
    static_assert(ITEMS % 2 == 1, "neighbouring lanes scan an odd number of words apart");
    static_assert((2 * TILE + 1 + WAVES) * 4 <= 32768, "five workgroups to the CU");
    __shared__ uint32_t slice[TILE + 1]; // slot k: offsets[a0 + k - 1]
    __shared__ uint32_t marks[TILE];     // word i: position b0 + i; after the scan, the slot of its segment's offset
    __shared__ uint32_t wave_top[WAVES];

    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint32_t num_segments = e.na - 1u;
    const MergeRanges r = expand_tile_ranges(e.split[t], e.split[t + 1], t, e.na + e.nb);
    const uint32_t na_t = r.a1 - r.a0, nb_t = r.b1 - r.b0; // na_t + nb_t <= TILE
    if (nb_t == 0u) return; // (workgroup-uniform) a tile of offsets alone: empty segments, or offsets at and beyond total

#pragma unroll
    for (uint32_t g = 0; g < ITEMS; g++) marks[g * kExpandThreads + tid] = 0u;
    for (uint32_t k = tid; k <= na_t; k += kExpandThreads)
    {
        bool has;
        const uint32_t at = expand_slice_source(r.a0, k, &has); // at < a1 <= na
        slice[k] = has ? e.offsets[at] : 0u;
    }
    __syncthreads();
    for (uint32_t k = tid + 1u; k <= na_t; k += kExpandThreads)
    {
        uint32_t at;
        if (expand_marks(k, na_t, slice[k], k < na_t ? slice[k + 1] : 0u, r.b0, nb_t, &at)) marks[at] = k;
    }
    __syncthreads();

    // the inclusive max-scan of the marks: ITEMS consecutive words per thread
    uint32_t m[ITEMS], run = 0u;
#pragma unroll
    for (uint32_t s = 0; s < ITEMS; s++)
    {
        const uint32_t v = marks[tid * ITEMS + s];
        run = run > v ? run : v;
        m[s] = run;
    }
    uint32_t before;
    const uint32_t top = wave_inclusive_max(run, before);
    if ((tid & 63u) == 63u) wave_top[tid / 64u] = top;
    __syncthreads();
#pragma unroll
    for (uint32_t w = 0; w + 1u < WAVES; w++)
    {
        const uint32_t v = wave_top[w];
        before = (w < tid / 64u && v > before) ? v : before;
    }
#pragma unroll
    for (uint32_t s = 0; s < ITEMS; s++) marks[tid * ITEMS + s] = m[s] > before ? m[s] : before; // (the thread's own words)
    __syncthreads();

    if (e.out_segments)
        expand_store_tile(marks, r.a0, num_segments, nb_t, e.out_segments + (size_t) r.b0,
                          [&](uint32_t, uint32_t segment, uint32_t) { return segment; });
    if (e.out_ranks)
        expand_store_tile(marks, r.a0, num_segments, nb_t, e.out_ranks + (size_t) r.b0,
                          [&](uint32_t i, uint32_t, uint32_t slot) { return r.b0 + i - slice[slot]; });
    if constexpr (ITEM_WORDS == 1)
        expand_store_tile(marks, r.a0, num_segments, nb_t, (uint32_t*) e.out_items + (size_t) r.b0,
                          [&](uint32_t, uint32_t segment, uint32_t) { return ((const uint32_t*) e.items)[segment]; });
    if constexpr (ITEM_WORDS == 2)
        expand_store_tile(marks, r.a0, num_segments, nb_t, (uint64_t*) e.out_items + (size_t) r.b0,
                          [&](uint32_t, uint32_t segment, uint32_t) { return ((const uint64_t*) e.items)[segment]; });
    if constexpr (ITEM_WORDS >= 4)
        expand_store_wide<ITEM_WORDS / 4>(marks, r.a0, num_segments, nb_t, (const Pack<uint32_t, 4>*) e.items,
                                          (Pack<uint32_t, 4>*) e.out_items + (size_t) r.b0 * (ITEM_WORDS / 4));
}

} // namespace glu_hip
