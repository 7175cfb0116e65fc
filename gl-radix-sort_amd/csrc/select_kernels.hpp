// select_kernels.hpp -- gfx950 kernels of SELECT (glu_select_run_ptr): stable stream compaction.  Element i is selected iff
// stencil[i] OP threshold holds; the indices of the selected elements, and the items at them, are written in ascending order of i.
// Not in the reference.
//
// The shape of key runs (key_runs_kernels.hpp) with another flag function.  Three kernels, whatever the stencil holds:
//   select_count_kernel   tile_counts[t] = selected elements of tile t.  A tile is SelectCfg::TILE elements: 256 threads x GROUPS
//                         packs of 16 bytes (four packs of 4- and 8-byte stencils, one pack of 16 byte stencils), wave-major, then
//                         pack, then lane, then the elements of a pack, so that the order of (wave, pack, lane, element) is the
//                         order of the elements.  Tiles are counted from the 16-byte boundary at or below `stencil`: every pack is
//                         aligned, whole packs take one 16-byte load, the packs that hold the first and the last element go
//                         element by element, and nothing outside the array is read.  One ballot + popcount per element position
//                         of a pack, the four wave sums through LDS, one barrier per tile (two rows of LDS in turn).
//   key_runs_scan_kernel  (key_runs_kernels.hpp, launched through host::launch_tile_count_scan) the counts scanned exclusively in
//                         place by one workgroup, the total written to *num_selected.
//   select_write_kernel   the flags of a tile again; the rank of a selected element = tile_counts[t] + the wave sums below its wave
//                         (LDS) + the selected elements below it in its wave (mbcnt of the ballots); out_indices[rank] = i and
//                         out_items[rank] = items[i] where rank < max_out.  An item is loaded where its flag is set and its rank is
//                         in range, and stored at once: no lane holds more than one item (two 16-byte words at most).
// OP is a run-time, workgroup-uniform argument, folded on the host into a SelectPred.  The stencil is read twice; nothing waits for
// another workgroup: no look-back, no atomics, no arrival order.  Both streaming kernels run a grid sized to the device and walk
// the tiles in a loop.
#pragma once

#include <type_traits>

#include "scan_batch_kernels.hpp"

namespace glu_hip
{
constexpr int kSelThreads = kSbThreads;
constexpr int kSelWaves = kSelThreads / kW;

enum
{
    SELECT_EQ = 0,
    SELECT_NE,
    SELECT_LT,
    SELECT_LE,
    SELECT_GT,
    SELECT_GE,
    SELECT_OPS_
};

template<typename S>
struct SelectCfg
{
    static constexpr uint32_t VEC = 16 / (uint32_t) sizeof(S);
    static constexpr uint32_t GROUPS = sizeof(S) == 1 ? 1 : 4; // packs per thread and tile
    static constexpr uint32_t WAVE_ELEMS = kW * GROUPS * VEC;
    static constexpr uint32_t TILE = kSelWaves * WAVE_ELEMS;
    static_assert(GROUPS * VEC <= 32, "a lane's flags are the bits of one word");
};

// The comparison of one call, folded on the host (make_select_pred).
// Integers (int32_t, uint32_t, uint8_t): every one of the six comparisons with a constant is "x lies in [a, b]" or its negation,
// in the order of the type.  With B = the sign bit of a signed type (0 of an unsigned one), x ^ B orders as unsigned and
// (x ^ B) - a == x - (a - B) modulo 2^32, so the test is ((uint32_t) x - lo) <= width with lo = a - B, width = b - a: a
// subtraction and an unsigned compare per element, which is what lets the byte stencil (16 elements per 16-byte load) keep up with
// its loads.
template<typename S>
struct SelectPred
{
    uint32_t lo, width, negate;
    __device__ __forceinline__ bool operator()(S x) const { return (((uint32_t) x - lo) <= width) != (negate != 0u); }
};

// Floats and doubles compare as IEEE values: x is below, equal to, above or unordered with the threshold (bits 0 .. 3), and `mask`
// holds the classes the comparison accepts.  A NaN on either side is unordered, which only NE accepts; -0.0 == +0.0.
template<typename S>
struct SelectPredIeee
{
    S threshold;
    uint32_t mask;
    __device__ __forceinline__ bool operator()(S x) const
    {
        const uint32_t cls = x < threshold ? 1u : x == threshold ? 2u : x > threshold ? 4u : 8u;
        return (mask & cls) != 0u;
    }
};
template<>
struct SelectPred<float> : SelectPredIeee<float>
{
};
template<>
struct SelectPred<double> : SelectPredIeee<double>
{
};

// host only: `op` (SELECT_EQ ..) against `threshold` as the predicate the kernels evaluate
template<typename S>
inline SelectPred<S> make_select_pred(int op, S threshold)
{
    SelectPred<S> p;
    if constexpr (std::is_floating_point<S>::value)
    {
        static const uint32_t masks[SELECT_OPS_] = {2u, 1u | 4u | 8u, 1u, 1u | 2u, 4u, 2u | 4u};
        p.threshold = threshold;
        p.mask = masks[op];
    }
    else
    {
        const uint32_t top = sizeof(S) == 1 ? 0xFFu : 0xFFFFFFFFu;     // the largest key
        const uint32_t bias = std::is_signed<S>::value ? 0x80000000u : 0u; // the sign bit of a signed type
        const uint32_t t = ((uint32_t) threshold & top) ^ bias;        // the threshold as an unsigned key
        uint32_t a = 0, b = top;                                       // [a, b] in key order; negate: its complement
        p.negate = 0;
        switch (op)
        {
        case SELECT_NE: p.negate = 1; [[fallthrough]];
        case SELECT_EQ: a = b = t; break;
        case SELECT_LT:
            if (t == 0) p.negate = 1; // (nothing is below the smallest key: the complement of everything)
            else b = t - 1;
            break;
        case SELECT_LE: b = t; break;
        case SELECT_GT:
            if (t == top) p.negate = 1;
            else a = t + 1;
            break;
        default: a = t; break; // SELECT_GE
        }
        p.lo = a - bias;
        p.width = b - a;
    }
    return p;
}

// host only: elements per tile, tiles of `count` elements from an aligned base (the rounds of the count scan:
// host::tile_count_scan_rounds)
inline void select_plan(uint64_t count, uint32_t stencil_bytes, uint32_t& tile, uint32_t& tiles)
{
    tile = stencil_bytes == 8 ? SelectCfg<uint64_t>::TILE : stencil_bytes == 1 ? SelectCfg<uint8_t>::TILE : SelectCfg<uint32_t>::TILE;
    tiles = (uint32_t) ((count + tile - 1) / tile);
}

// What a call passes to its two streaming kernels.  `base` is the 16-byte boundary at or below the stencil; the stencil is the
// elements [lo, hi) of it (lo < VEC).
template<typename S>
struct SelectArgs
{
    const S* base;
    uint64_t lo, hi;
    SelectPred<S> pred;
    uint32_t tiles;
};

// The flags of the calling lane's elements of tile `t`: bit g * VEC + k for element k of the lane's pack g.  Elements outside
// [lo, hi) are not read and not selected.  first = the lane's pack 0 as an element of `base`; pack g: + g * kW * VEC.
template<typename S>
__device__ __forceinline__ uint32_t select_flags(const SelectArgs<S>& a, uint32_t t, uint32_t wave, uint32_t lane, uint64_t& first)
{
    using C = SelectCfg<S>;
    first = (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC;
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::GROUPS; g++)
    {
        const uint64_t v0 = first + g * kW * C::VEC;
        if (v0 >= a.lo && v0 + C::VEC <= a.hi)
        {
            const Pack<S, C::VEC> pk = *reinterpret_cast<const Pack<S, C::VEC>*>(a.base + v0);
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++) flags |= (a.pred(pk.v[k]) ? 1u : 0u) << (g * C::VEC + k);
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++)
                if (v0 + k >= a.lo && v0 + k < a.hi) flags |= (a.pred(a.base[v0 + k]) ? 1u : 0u) << (g * C::VEC + k);
        }
    }
    return flags;
}

template<typename S>
__global__ __launch_bounds__(kSelThreads) void select_count_kernel(SelectArgs<S> a, uint32_t* __restrict__ tile_counts)
{
    using C = SelectCfg<S>;
    __shared__ uint32_t wsum[2][kSelWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t phase = 0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        uint64_t first;
        const uint32_t flags = select_flags(a, t, wave, lane, first);
        uint32_t n = 0;
#pragma unroll
        for (uint32_t b = 0; b < C::GROUPS * C::VEC; b++) n += (uint32_t) __popcll(__ballot((flags >> b) & 1u));
        uint32_t* row = wsum[phase & 1u];
        phase++;
        if (lane == 0) row[wave] = n;
        __syncthreads();
        if (threadIdx.x == 0)
        {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < kSelWaves; w++) sum += row[w];
            tile_counts[t] = sum;
        }
    }
}

// An item of ITEM_BYTES (4, 8, 16 or 32) bytes, copied bit for bit; 16 and 32 bytes move as 16-byte words.
template<uint32_t ITEM_BYTES>
struct SelectItem
{
    using Word = uint4;
};
template<>
struct SelectItem<4>
{
    using Word = uint32_t;
};
template<>
struct SelectItem<8>
{
    using Word = uint64_t;
};

// ITEM_BYTES == 0: no items (indices only).  out_indices may be NULL where ITEM_BYTES != 0.
template<typename S, uint32_t ITEM_BYTES>
__global__ __launch_bounds__(kSelThreads) void select_write_kernel(SelectArgs<S> a, const uint32_t* __restrict__ tile_counts,
                                                                   const void* __restrict__ items, void* __restrict__ out_items,
                                                                   uint32_t* __restrict__ out_indices, uint32_t max_out)
{
    using C = SelectCfg<S>;
    using Word = typename SelectItem<ITEM_BYTES>::Word;
    constexpr uint32_t WORDS = ITEM_BYTES ? ITEM_BYTES / (uint32_t) sizeof(Word) : 0u;
    __shared__ uint32_t wsum[2][kSelWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t phase = 0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        uint64_t first;
        const uint32_t flags = select_flags(a, t, wave, lane, first);
        uint32_t below[C::GROUPS]; // selected elements of the wave in front of the lane's pack g
        uint32_t wave_total = 0;
#pragma unroll
        for (uint32_t g = 0; g < C::GROUPS; g++)
        {
            uint32_t mine = 0, all = 0;
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++)
            {
                const uint64_t b = __ballot((flags >> (g * C::VEC + k)) & 1u);
                mine += __builtin_amdgcn_mbcnt_hi((uint32_t) (b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) b, 0u));
                all += (uint32_t) __popcll(b);
            }
            below[g] = wave_total + mine;
            wave_total += all;
        }
        uint32_t* row = wsum[phase & 1u];
        phase++;
        if (lane == 0) row[wave] = wave_total;
        __syncthreads();
        uint32_t base = tile_counts[t];
#pragma unroll
        for (int w = 0; w < kSelWaves; w++)
            if ((uint32_t) w < wave) base += row[w];
#pragma unroll
        for (uint32_t g = 0; g < C::GROUPS; g++)
        {
            // (mbcnt counted the lanes below for every element position: the lane's own earlier elements of the pack are added here)
            uint32_t rank = base + below[g];
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++)
            {
                if ((flags >> (g * C::VEC + k)) & 1u)
                {
                    if (rank < max_out)
                    {
                        const uint32_t i = (uint32_t) (first + g * kW * C::VEC + k - a.lo);
                        if (out_indices) out_indices[rank] = i;
                        if constexpr (ITEM_BYTES != 0)
                        {
                            const Word* src = reinterpret_cast<const Word*>(items) + (uint64_t) i * WORDS;
                            Word* dst = reinterpret_cast<Word*>(out_items) + (uint64_t) rank * WORDS;
#pragma unroll
                            for (uint32_t w = 0; w < WORDS; w++) dst[w] = src[w];
                        }
                    }
                    rank++;
                }
            }
        }
    }
}

} // namespace glu_hip
