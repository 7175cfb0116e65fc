// select_batch_kernels.hpp -- gfx950 kernels of the BATCHED SELECT (glu_select_run_batch_ptr, glu_select_run_batch_offsets_ptr):
// the single call's compaction (select_kernels.hpp over tile_compact_kernels.hpp) of the elements between the first and the last
// boundary of a list of segments, plus what the single call lacks: the offsets of the compacted segments, and indices local to a
// selected element's segment.  Not in the reference.
//   count    select_batch_count_kernel: the flags of a tile as select_count_kernel makes them, masked to [b_0, b_n) from two loads of
//            the offsets; besides the count of the tile it stores what it already holds: every lane's flag word and the wave sums
//            below each wave (select_batch_rank.hpp states the layout).  A tile outside [b_0, b_n) is not read.
//   scan     key_runs_scan_kernel over tiles + 1 counts (the last one a zero), so that entry `tiles` becomes the total.
//   offsets  select_batch_offsets_kernel: one thread per boundary, out_offsets[s] = min(max_out, select_batch_rank(b_s)): a count, a
//            wave sum and one wave's flag words under a mask -- two or three cache lines per boundary whatever the data hold, so 2^24
//            empty segments at one position are 2^24 threads that read the same lines.
//   write    select_batch_write_kernel: tile_compact on the STORED flag words -- the stencil is read once by the batched call, and
//            this kernel depends on the stencil's width alone.  A tile with nothing selected is skipped.  In LOCAL form a selected
//            element finds its segment by a bound over the offsets between the segments of the tile's first and last element,
//            which two workgroup-uniform searches find (how the batched sorted search finds a needle's segment; here the 64 lanes
//            of every wave probe together, four rounds for 2^24 segments); a tile inside one segment searches no further, a tile
//            of up to 256 segments searches a copy of their offsets in LDS, and with equal partitions the index is a remainder.  The form is a template argument.
// Nothing waits for another workgroup: no look-back, no atomics, nothing in arrival order; the grids follow from the counts.
#pragma once

#include "select_batch_rank.hpp"
#include "select_kernels.hpp"

namespace glu_hip
{
enum
{
    SELECT_INDEX_GLOBAL = 0,
    SELECT_INDEX_LOCAL,
    SELECT_INDEX_FORMS_
};

template<typename S>
using SelectBatchCfgOf = SelectBatchCfg<sizeof(S), select_packs(sizeof(S))>;

template<uint32_t LANE_BITS>
struct SelectFlagWord
{
    using type = uint16_t;
};
template<>
struct SelectFlagWord<8>
{
    using type = uint8_t;
};

// The segments of a call: device offsets (num_segments + 1 of them), or equal partitions of `count` where offsets == nullptr.
struct SelectBatchSegs
{
    const uint32_t* offsets;
    uint32_t num_segments, count, total;

    // b_s, s <= num_segments
    __device__ __forceinline__ uint32_t boundary(uint32_t s) const
    {
        if (!offsets) return s * count;
        const uint32_t o = offsets[s];
        return o < total ? o : total;
    }
};

// What the three kernels share of the call's scratch (select_batch_scratch).
struct SelectBatchScratchPtrs
{
    uint32_t* tile_counts; // tiles + 1
    uint32_t* wave_below;  // 4 per tile
    void* flags;           // a flag word per thread and tile
};

template<typename S>
__global__ __launch_bounds__(kTileThreads) void select_batch_count_kernel(SelectArgs<S> a, SelectBatchSegs segs, SelectBatchScratchPtrs scratch)
{
    using C = SelectBatchCfgOf<S>;
    using Flag = typename SelectFlagWord<C::LANE_BITS>::type;
    TileWalk<SelectCfg<S>> w;
    // the selected range as elements of the span's base (empty where the offsets decrease: first >= last)
    const uint64_t first = a.stencil.lo + segs.boundary(0), last = a.stencil.lo + segs.boundary(segs.num_segments);
    if (blockIdx.x == 0 && threadIdx.x == 0) scratch.tile_counts[a.stencil.tiles] = 0; // (the count scan turns it into the total)
    for (uint32_t t = blockIdx.x; t < a.stencil.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        const uint64_t tile0 = (uint64_t) t * C::TILE, tile1 = tile0 + C::TILE;
        uint32_t f = 0;
        if (tile1 > first && tile0 < last) // (workgroup-uniform)
        {
            const uint64_t mine = w.first(t);
            f = select_flags(a, mine);
            if (tile0 < first || tile1 > last)
            {
                uint32_t inside = 0;
#pragma unroll
                for (uint32_t g = 0; g < C::PACKS; g++)
#pragma unroll
                    for (uint32_t k = 0; k < C::VEC; k++)
                    {
                        const uint64_t v = mine + g * C::PACK_STRIDE + k;
                        inside |= (v >= first && v < last ? 1u : 0u) << (g * C::VEC + k);
                    }
                f &= inside;
            }
        }
        reinterpret_cast<Flag*>(scratch.flags)[(size_t) t * kTileThreads + threadIdx.x] = (Flag) f;
        // tile_count, which also keeps the wave sums below each wave
        uint32_t n = 0;
#pragma unroll
        for (uint32_t b = 0; b < C::LANE_BITS; b++) n += (uint32_t) __popcll(__ballot((f >> b) & 1u));
        uint32_t* row = w.row();
        if (w.lane == 0) row[w.wave] = n;
        __syncthreads();
        if (threadIdx.x == 0)
        {
            uint4 below;
            below.x = 0;
            below.y = row[0];
            below.z = below.y + row[1];
            below.w = below.z + row[2];
            reinterpret_cast<uint4*>(scratch.wave_below)[t] = below;
            scratch.tile_counts[t] = below.w + row[3];
        }
    }
}
static_assert(kTileWaves == 4, "the wave sums below the waves of a tile are one uint4");

template<uint32_t ELEM_BYTES>
__global__ __launch_bounds__(256) void select_batch_offsets_kernel(SelectBatchSegs segs, uint64_t lo, uint32_t tiles, SelectBatchScratchPtrs scratch,
                                                                   uint32_t* __restrict__ out_offsets, uint32_t max_out)
{
    using C = SelectBatchCfg<ELEM_BYTES, select_packs(ELEM_BYTES)>;
    const uint64_t* words = reinterpret_cast<const uint64_t*>(scratch.flags);
    for (uint64_t s = (uint64_t) blockIdx.x * 256u + threadIdx.x; s <= segs.num_segments; s += (uint64_t) gridDim.x * 256u)
    {
        const uint32_t rank = select_batch_rank<C>(lo + segs.boundary((uint32_t) s), tiles, scratch.tile_counts, scratch.wave_below,
                                                   [&](size_t i) { return words[i]; });
        out_offsets[s] = rank < max_out ? rank : max_out;
    }
}

// the last s in [lo, hi] with offsets[s] <= i (lo where there is none): every read lies in [lo, hi], whatever the offsets hold
__device__ __forceinline__ uint32_t select_batch_last_le(const uint32_t* __restrict__ offsets, uint32_t lo, uint32_t hi, uint32_t i)
{
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// The same for two elements at once over all of [0, n], by the 64 lanes of a wave together: every round a lane probes one of 64
// evenly spaced offsets for each element, and the ballots narrow both ranges 64-fold -- four rounds of two loads for 2^24 segments
// where the binary search takes 24 dependent loads each.  The trip count follows from n alone (wave-uniform, and the same for both
// elements); every probe lies in [0, n] and so does the result, whatever the offsets hold.
__device__ __forceinline__ void select_batch_wave_last_le(const uint32_t* __restrict__ offsets, uint32_t n, uint32_t lane, uint32_t ia, uint32_t ib,
                                                          uint32_t& sa, uint32_t& sb)
{
    sa = sb = 0;
    for (uint32_t len = n; len != 0;)
    {
        const uint32_t step = (len + 63u) / 64u; // the answers lie in [sa, sa + len] and [sb, sb + len]
        const uint32_t pa = sa + (lane + 1u) * step, pb = sb + (lane + 1u) * step;
        const bool a = pa <= n && offsets[pa <= n ? pa : n] <= ia, b = pb <= n && offsets[pb <= n ? pb : n] <= ib;
        sa += (uint32_t) __popcll(__ballot(a)) * step; // (a probe that passed lies at or below n: so does the sum)
        sb += (uint32_t) __popcll(__ballot(b)) * step;
        len = step - 1u;
    }
}

constexpr uint32_t kSelectBatchSlice = kTileThreads; // offsets of a tile kept in LDS: one load per thread

// ITEM_BYTES == 0: no items (indices only).  out_indices may be NULL where ITEM_BYTES != 0.
template<uint32_t ELEM_BYTES, uint32_t ITEM_BYTES, bool LOCAL>
__global__ __launch_bounds__(kTileThreads) void select_batch_write_kernel(SelectBatchSegs segs, uint64_t lo, uint32_t tiles, SelectBatchScratchPtrs scratch,
                                                                          const void* __restrict__ items, void* __restrict__ out_items,
                                                                          uint32_t* __restrict__ out_indices, uint32_t max_out)
{
    using C = SelectBatchCfg<ELEM_BYTES, select_packs(ELEM_BYTES)>;
    using Flag = typename SelectFlagWord<C::LANE_BITS>::type;
    using Word = typename SelectItem<ITEM_BYTES>::Word;
    constexpr uint32_t WORDS = ITEM_BYTES ? ITEM_BYTES / (uint32_t) sizeof(Word) : 0u;
    TileWalk<TileCfg<ELEM_BYTES, select_packs(ELEM_BYTES)>> w;
    TileSpan<uint8_t> span; // (tile_compact takes the first element of the array from it)
    span.base = nullptr;
    span.lo = lo;
    span.hi = lo + segs.total;
    span.tiles = tiles;
    const uint32_t* __restrict__ tile_scan = scratch.tile_counts;
    uint32_t slice_phase = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) // (workgroup-uniform)
    {
        const uint32_t below = tile_scan[t];
        if (tile_scan[t + 1] == below || below >= max_out) continue; // (workgroup-uniform: nothing selected, or no room left for it)
        const uint32_t f = reinterpret_cast<const Flag*>(scratch.flags)[(size_t) t * kTileThreads + threadIdx.x];
        uint32_t seg_lo = 0, seg_hi = 0, seg_lo_begin = 0;
        const uint32_t* slice = nullptr; // offsets[seg_lo .. seg_hi] in LDS, where the tile holds few enough segments
        if constexpr (LOCAL)
        {
            // two slices in turn, as the rows of the walk: the barrier of the next tile's tile_compact lies between the reads of one
            // tile and the writes of the tile after the next
            __shared__ uint32_t slices[2][kSelectBatchSlice];
            if (segs.offsets) // (workgroup-uniform, as the two searches and their results are)
            {
                const uint64_t tile0 = (uint64_t) t * C::TILE, tile1 = tile0 + C::TILE;
                const uint32_t i_first = (uint32_t) ((tile0 > span.lo ? tile0 : span.lo) - span.lo);
                const uint32_t i_last = (uint32_t) ((tile1 < span.hi ? tile1 : span.hi) - 1u - span.lo);
                select_batch_wave_last_le(segs.offsets, segs.num_segments, w.lane, i_first, i_last, seg_lo, seg_hi);
                if (seg_hi < seg_lo) seg_hi = seg_lo; // (offsets that decrease)
                seg_lo_begin = segs.offsets[seg_lo];
                if (seg_hi != seg_lo && seg_hi - seg_lo < kSelectBatchSlice)
                {
                    uint32_t* mine = slices[slice_phase++ & 1u];
                    if (threadIdx.x <= seg_hi - seg_lo) mine[threadIdx.x] = segs.offsets[seg_lo + threadIdx.x];
                    slice = mine; // (read behind the barrier of tile_compact)
                }
            }
        }
        tile_compact(w, t, f, span, tile_scan, [&](uint32_t rank, uint32_t, uint32_t, uint32_t i) {
            if (rank < max_out)
            {
                if (out_indices)
                {
                    uint32_t index = i;
                    if constexpr (LOCAL)
                    {
                        if (!segs.offsets) index = i % segs.count;
                        else if (seg_lo == seg_hi) index = i - seg_lo_begin; // (the whole tile lies in one segment)
                        else if (slice) index = i - slice[select_batch_last_le(slice, 0u, seg_hi - seg_lo, i)];
                        else index = i - segs.offsets[select_batch_last_le(segs.offsets, seg_lo, seg_hi, i)];
                    }
                    out_indices[rank] = index;
                }
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
}

} // namespace glu_hip
