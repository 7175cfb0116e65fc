// select_kernels.hpp -- gfx950 kernels of SELECT (glu_select_run_ptr): stable stream compaction.  Element i is selected iff
// stencil[i] OP threshold holds; the indices of the selected elements, and the items at them, are written in ascending order of i.
// Not in the reference.
//
// Select is a flag-and-compact operator (tile_compact_kernels.hpp: the tiles, the load of a pack, the count per tile, the ranks);
// what it adds:
//   the flags   select_flags: a predicate on the element.  OP is a run-time, workgroup-uniform argument, folded on the host into a
//               SelectPred, and evaluated only on elements of the array: a zero read as padding would pass EQ 0.
//   the tile    four packs of 4- and 8-byte stencils per thread, one pack of 16 byte stencils.
//   the write   out_indices[rank] = i and out_items[rank] = items[i] where rank < max_out.  An item is loaded where its flag is set
//               and its rank is in range, and stored at once: no lane holds more than one item (two 16-byte words at most).
// The stencil is read twice.
#pragma once

#include <type_traits>

#include "tile_compact_kernels.hpp"

namespace glu_hip
{
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

// packs per thread and tile
constexpr uint32_t select_packs(uint32_t stencil_bytes) { return stencil_bytes == 1 ? 1u : 4u; }
template<typename S>
using SelectCfg = TileCfg<sizeof(S), select_packs(sizeof(S))>;

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

// What a call passes to its two streaming kernels.
template<typename S>
struct SelectArgs
{
    TileSpan<S> stencil;
    SelectPred<S> pred;
};

// The flags of the calling lane's elements of a tile (`first`: its pack 0).  Elements outside the array are not selected.
template<typename S>
__device__ __forceinline__ uint32_t select_flags(const SelectArgs<S>& a, uint64_t first)
{
    using C = SelectCfg<S>;
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
        tile_load_pack<C::VEC>(a.stencil, first + g * C::PACK_STRIDE, [&](uint32_t k, S x, bool inside) {
            if (inside) flags |= (a.pred(x) ? 1u : 0u) << (g * C::VEC + k);
        });
    return flags;
}

template<typename S>
__global__ __launch_bounds__(kTileThreads) void select_count_kernel(SelectArgs<S> a, uint32_t* __restrict__ tile_counts)
{
    TileWalk<SelectCfg<S>> w;
    for (uint32_t t = blockIdx.x; t < a.stencil.tiles; t += gridDim.x) // (workgroup-uniform)
        tile_count(w, t, select_flags(a, w.first(t)), tile_counts);
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
__global__ __launch_bounds__(kTileThreads) void select_write_kernel(SelectArgs<S> a, const uint32_t* __restrict__ tile_counts,
                                                                    const void* __restrict__ items, void* __restrict__ out_items,
                                                                    uint32_t* __restrict__ out_indices, uint32_t max_out)
{
    using Word = typename SelectItem<ITEM_BYTES>::Word;
    constexpr uint32_t WORDS = ITEM_BYTES ? ITEM_BYTES / (uint32_t) sizeof(Word) : 0u;
    TileWalk<SelectCfg<S>> w;
    for (uint32_t t = blockIdx.x; t < a.stencil.tiles; t += gridDim.x) // (workgroup-uniform)
        tile_compact(w, t, select_flags(a, w.first(t)), a.stencil, tile_counts, [&](uint32_t rank, uint32_t, uint32_t, uint32_t i) {
            if (rank < max_out)
            {
                if (out_indices) out_indices[rank] = i;
                if constexpr (ITEM_BYTES != 0)
                {
                    const Word* src = reinterpret_cast<const Word*>(items) + (uint64_t) i * WORDS;
                    Word* dst = reinterpret_cast<Word*>(out_items) + (uint64_t) rank * WORDS;
#pragma unroll
                    for (uint32_t n = 0; n < WORDS; n++) dst[n] = src[n];
                }
            }
        });
}

} // namespace glu_hip
