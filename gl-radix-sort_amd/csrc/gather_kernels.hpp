// gather_kernels.hpp -- gfx950 kernels of GATHER and SCATTER (glu_gather.hip): items fetched or placed by device indices.  Not in
// the reference.
//   gather_kernel<B, false>   out[j] = items[indices[j]]                         where indices[j] < item_count
//   gather_kernel<B, true>    out[s * k + c] = items[begin_s + indices[s * k + c]]  where c < min(k, len_s) and the index < len_s
//   scatter_kernel<B>         out[indices[j]] = items[j]                         where indices[j] < out_count
// Entries that fail their test are not touched.  B = item_bytes, 4, 8, 16 or 32.
//
// The calls are bound by the memory system's answer to scattered accesses of 4 to 32 bytes; the kernels keep everything around those
// accesses out of the way.  One workgroup of 256 per tile, no LDS, no atomics, nothing waits for another workgroup.  The STREAMING
// SIDE (out of a gather, items of a scatter) moves in whole 16-byte packs by contiguous lanes whatever the alignment of the array:
// packs are counted from the 16-byte boundary at or below it (gather_walk.hpp over tile_span.hpp), a 32-byte item is two packs in
// two neighbouring lanes, and a pack goes element by element only where it holds an end of the array or an entry that stays
// untouched.  A lane issues all of its index loads, then all of its item loads (PACKS x 16 / min(B, 16) of each), then stores: the
// scattered loads of a lane are in flight together.  A tile that lies inside the array (every tile of a call but the first and the
// last; workgroup-uniform) tests no piece against the array's ends, which is what lets its index loads leave back to back; the other
// two run the same code with the tests.  Indices and the streaming side go through the streaming forms of
// device_utils.hpp, so that what the caches hold is the table.  Which memory an entry may touch is gather_walk.hpp's, plain C++
// tested on the host: no index and no offset is trusted.
#pragma once

#include "device_utils.hpp"
#include "gather_walk.hpp"

namespace glu_hip
{
struct GatherArgs
{
    const void* items;
    const uint32_t* indices;
    void* out;
    const uint32_t* offsets; // batched, offsets form: num_segments + 1 words
    uint64_t lo, hi;         // the streaming side is the pieces [lo, hi) of its aligned base
    uint64_t bound;          // item_count of a gather, out_count of a scatter
    GatherRows rows;         // batched
};

typedef uint32_t gather_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));

template<uint32_t PIECE_BYTES>
struct GatherPiece;
template<>
struct GatherPiece<4>
{
    typedef uint32_t type;
};
template<>
struct GatherPiece<8>
{
    typedef uint64_t type;
};
template<>
struct GatherPiece<16>
{
    typedef gather_u32x4 type;
};

template<typename Piece, uint32_t VEC>
struct alignas(16) GatherPack
{
    Piece v[VEC];
};

template<typename Cfg>
__device__ __forceinline__ bool gather_indices_aligned(const GatherArgs& a)
{
    return Cfg::VEC > 1u && ((uintptr_t) a.indices - a.lo * sizeof(uint32_t)) % (Cfg::VEC * sizeof(uint32_t)) == 0u;
}

// Every index word of the lane: idx[g][k] and inside[g][k] for the VEC pieces of its PACKS packs.  INTERIOR: every piece of the tile
// is one of the array (gather_tile_inside; all tiles but the first and the last of a call), so nothing is tested and the loads leave
// back to back: one streaming load a pack where the index array is aligned like the packs (kernel-uniform), else one a word.
// Otherwise a piece outside the array loads nothing.
template<typename Cfg, bool INTERIOR>
__device__ __forceinline__ void gather_load_indices(const GatherArgs& a, uint32_t wave, uint32_t lane, uint32_t (&idx)[Cfg::PACKS][Cfg::VEC],
                                                    bool (&inside)[Cfg::PACKS][Cfg::VEC])
{
    constexpr uint32_t VEC = Cfg::VEC, PACKS = Cfg::PACKS;
    if (INTERIOR && gather_indices_aligned<Cfg>(a))
    {
#pragma unroll
        for (uint32_t g = 0; g < PACKS; g++)
        {
            const uint32_t* at = a.indices + (gather_pack_first<Cfg>(blockIdx.x, wave, g, lane) - a.lo);
            if constexpr (VEC == 4)
            {
                const gather_u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const gather_u32x4*>(at));
                idx[g][0] = r.x, idx[g][1] = r.y, idx[g][2] = r.z, idx[g][3] = r.w;
            }
            if constexpr (VEC == 2)
            {
                const gather_u32x2 r = __builtin_nontemporal_load(reinterpret_cast<const gather_u32x2*>(at));
                idx[g][0] = r.x, idx[g][1] = r.y;
            }
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++) inside[g][k] = true;
        }
        return;
    }
#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
    {
        const uint64_t first = gather_pack_first<Cfg>(blockIdx.x, wave, g, lane);
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            inside[g][k] = INTERIOR || gather_inside(first + k, a.lo, a.hi);
            uint32_t item = 0u, part;
            if (inside[g][k]) gather_item_of(first + k, a.lo, Cfg::PIECES, &item, &part);
            idx[g][k] = inside[g][k] ? __builtin_nontemporal_load(a.indices + item) : 0u;
        }
    }
}

template<uint32_t ITEM_BYTES, bool BATCH, bool INTERIOR>
__device__ __forceinline__ void gather_tile(const GatherArgs& a)
{
    using Cfg = GatherCfg<ITEM_BYTES>;
    using Piece = typename GatherPiece<Cfg::PIECE_BYTES>::type;
    constexpr uint32_t VEC = Cfg::VEC, PACKS = Cfg::PACKS, PIECES = Cfg::PIECES;
    const uint32_t wave = threadIdx.x / kTileLanes, lane = threadIdx.x % kTileLanes;
    Piece* base = (Piece*) a.out - a.lo; // the 16-byte boundary at or below out
    const Piece* items = (const Piece*) a.items;

    // every index of the lane
    uint32_t idx[PACKS][VEC];
    bool live[PACKS][VEC];
    gather_load_indices<Cfg, INTERIOR>(a, wave, lane, idx, live);

    // where each entry comes from, in pieces of the table
    uint64_t from[PACKS][VEC];
#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
    {
        const uint64_t first = gather_pack_first<Cfg>(blockIdx.x, wave, g, lane);
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            uint32_t j = 0u, part = 0u, source = 0u;
            if (live[g][k]) gather_item_of(first + k, a.lo, PIECES, &j, &part);
            if constexpr (BATCH)
            {
                uint32_t s, col, begin, len;
                gather_row(j, a.rows, &s, &col); // s < num_segments: j < num_segments * k
                if (a.rows.offsets_form)         // (kernel-uniform)
                {
                    const uint32_t b = live[g][k] ? a.offsets[s] : 0u, e = live[g][k] ? a.offsets[s + 1u] : 0u;
                    gather_offsets_segment(b, e, a.rows, &begin, &len);
                }
                else
                    gather_partition_segment(s, a.rows, &begin, &len);
                live[g][k] = gather_batch_source(begin, len, col, idx[g][k], a.rows, &source) && live[g][k];
            }
            else
            {
                live[g][k] = live[g][k] && idx[g][k] < a.bound;
                source = idx[g][k];
            }
            from[g][k] = (uint64_t) source * PIECES + part;
        }
    }

    // every item of the lane
    Piece v[PACKS][VEC];
#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++) v[g][k] = live[g][k] ? items[from[g][k]] : Piece();

#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
    {
        const uint64_t first = gather_pack_first<Cfg>(blockIdx.x, wave, g, lane);
        bool whole = INTERIOR || gather_pack_inside(first, VEC, a.lo, a.hi);
        GatherPack<Piece, VEC> pack;
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            whole = whole && live[g][k];
            pack.v[k] = v[g][k];
        }
        if (whole)
            store_streaming(reinterpret_cast<GatherPack<Piece, VEC>*>(base + first), pack);
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++)
                if (live[g][k]) base[first + k] = v[g][k];
        }
    }
}

// (workgroup-uniform: the first and the last tile of a call take the tested form)
template<uint32_t ITEM_BYTES, bool BATCH>
__global__ __launch_bounds__(kGatherThreads) void gather_kernel(GatherArgs a)
{
    if (gather_tile_inside(blockIdx.x, GatherCfg<ITEM_BYTES>::TILE, a.lo, a.hi))
        gather_tile<ITEM_BYTES, BATCH, true>(a);
    else
        gather_tile<ITEM_BYTES, BATCH, false>(a);
}

template<uint32_t ITEM_BYTES, bool INTERIOR>
__device__ __forceinline__ void scatter_tile(const GatherArgs& a)
{
    using Cfg = GatherCfg<ITEM_BYTES>;
    using Piece = typename GatherPiece<Cfg::PIECE_BYTES>::type;
    constexpr uint32_t VEC = Cfg::VEC, PACKS = Cfg::PACKS, PIECES = Cfg::PIECES;
    const uint32_t wave = threadIdx.x / kTileLanes, lane = threadIdx.x % kTileLanes;
    const Piece* base = (const Piece*) a.items - a.lo; // the 16-byte boundary at or below items
    Piece* out = (Piece*) a.out;

    uint32_t idx[PACKS][VEC];
    bool live[PACKS][VEC];
    gather_load_indices<Cfg, INTERIOR>(a, wave, lane, idx, live);

    Piece v[PACKS][VEC];
#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
    {
        const uint64_t first = gather_pack_first<Cfg>(blockIdx.x, wave, g, lane);
        if (INTERIOR || gather_pack_inside(first, VEC, a.lo, a.hi))
        {
            const GatherPack<Piece, VEC> pack = load_streaming(reinterpret_cast<const GatherPack<Piece, VEC>*>(base + first));
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++) v[g][k] = pack.v[k];
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++) v[g][k] = live[g][k] ? base[first + k] : Piece();
        }
    }

#pragma unroll
    for (uint32_t g = 0; g < PACKS; g++)
    {
        const uint64_t first = gather_pack_first<Cfg>(blockIdx.x, wave, g, lane);
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            uint32_t j = 0u, part = 0u;
            if (live[g][k]) gather_item_of(first + k, a.lo, PIECES, &j, &part);
            if (live[g][k] && idx[g][k] < a.bound) out[(uint64_t) idx[g][k] * PIECES + part] = v[g][k];
        }
    }
}

template<uint32_t ITEM_BYTES>
__global__ __launch_bounds__(kGatherThreads) void scatter_kernel(GatherArgs a)
{
    if (gather_tile_inside(blockIdx.x, GatherCfg<ITEM_BYTES>::TILE, a.lo, a.hi))
        scatter_tile<ITEM_BYTES, true>(a);
    else
        scatter_tile<ITEM_BYTES, false>(a);
}

} // namespace glu_hip
