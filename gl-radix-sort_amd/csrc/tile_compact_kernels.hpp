// tile_compact_kernels.hpp -- the device half of the flag-and-compact operators (key runs, select), written once.  An operator
// flags the elements of an array, tile by tile (tile_span.hpp), and says what is written for a flagged element.  Its kernels:
//   count   tile_counts[t] = flags of tile t (tile_count).  One ballot + popcount per element position of a pack, the four wave
//           sums through LDS, one barrier per tile (two rows of LDS in turn, as in scan_batch_range).
//   scan    key_runs_scan_kernel (tile_count_scan_kernel.hpp), one workgroup: the counts scanned exclusively in place.
//   write   the flags of a tile again (tile_compact); the rank of a flagged element = tile_counts[t] + the wave sums below its wave
//           (LDS) + the flagged elements below it in its wave (mbcnt of the ballots); the operator's emit for every flagged
//           element, in ascending order.  Whether a rank is in range is the operator's to test.
// The seam is the flags of a whole tile, not the flag of one element (key runs carries the key in front of a pack from lane to
// lane and keeps the keys in registers): a lane's flags are one word, bit g * VEC + k for element k of its pack g.  The operator's
// __global__ kernels own the loop over the tiles and call their flag function in it themselves; everything here
// is inlined into them.  The array is read twice; nothing waits for another workgroup: no look-back, no atomics, no arrival order.
// The grids are sized to the device.
#pragma once

#include "scan_batch_kernels.hpp"
#include "tile_span.hpp"

namespace glu_hip
{
static_assert(kTileLanes == kW && kTileThreads == kSbThreads && kTileScanRound == ScanCfg<uint32_t, 4, kSbThreads>::CHUNK,
              "tile_span.hpp states the wave, the workgroup and the round of the count scan for itself");

// The pack at element v0 of the span's base: f(k, element, inside) for k = 0 .. VEC - 1.  A pack that lies wholly inside [lo, hi)
// takes one aligned 16-byte load; the packs that hold the first and the last element go element by element, and an element outside
// the array is not read: f gets a zero and inside == false.
template<uint32_t VEC, typename T, typename F>
__device__ __forceinline__ void tile_load_pack(const TileSpan<T>& s, uint64_t v0, F f)
{
    if (v0 >= s.lo && v0 + VEC <= s.hi)
    {
        const Pack<T, VEC> pk = *reinterpret_cast<const Pack<T, VEC>*>(s.base + v0);
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++) f(k, pk.v[k], true);
    }
    else
    {
#pragma unroll
        for (uint32_t k = 0; k < VEC; k++)
        {
            const bool inside = v0 + k >= s.lo && v0 + k < s.hi;
            f(k, inside ? s.base[v0 + k] : (T) 0, inside);
        }
    }
}

// What a workgroup keeps over its loop for (t = blockIdx.x; t < tiles; t += gridDim.x): the kernel flags tile t and hands the flags
// to tile_count or tile_compact, which take one barrier per tile and two rows of LDS in turn.  The rows are the workgroup's, declared
// in row(): a kernel has ONE walk (two TileWalk<C> of the same C in one kernel would share them and need a barrier of their own).
template<typename C>
struct TileWalk
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t phase = 0;

    // the calling lane's pack 0 of tile t, as an element of the span's base
    __device__ __forceinline__ uint64_t first(uint32_t t) const { return (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC; }

    // the wave sums of this tile: a row of LDS, the other one than the tile before
    __device__ __forceinline__ uint32_t* row()
    {
        __shared__ uint32_t wsum[2][kTileWaves];
        return wsum[phase++ & 1u];
    }
};

// tile_counts[t] = flags of tile t, `f` being the calling lane's
template<typename C>
__device__ __forceinline__ void tile_count(TileWalk<C>& w, uint32_t t, uint32_t f, uint32_t* tile_counts)
{
    uint32_t n = 0;
#pragma unroll
    for (uint32_t b = 0; b < C::PACKS * C::VEC; b++) n += (uint32_t) __popcll(__ballot((f >> b) & 1u));
    uint32_t* row = w.row();
    if (w.lane == 0) row[w.wave] = n;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < kTileWaves; i++) sum += row[i];
        tile_counts[t] = sum;
    }
}

// emit(rank, g, k, i) for every flagged element of tile t (element k of the lane's pack g, element i of the array), in ascending order
template<typename C, typename T, typename Emit>
__device__ __forceinline__ void tile_compact(TileWalk<C>& w, uint32_t t, uint32_t f, const TileSpan<T>& s, const uint32_t* tile_counts,
                                             Emit emit)
{
    const uint32_t i0 = (uint32_t) (w.first(t) - s.lo); // the lane's pack 0 as an element of the array (modulo 2^32 in front of it)
    uint32_t below[C::PACKS]; // flags of the wave in front of the lane's pack g
    uint32_t wave_total = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
    {
        uint32_t mine = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < C::VEC; k++)
        {
            const uint64_t b = __ballot((f >> (g * C::VEC + k)) & 1u);
            mine += __builtin_amdgcn_mbcnt_hi((uint32_t) (b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) b, 0u));
            all += (uint32_t) __popcll(b);
        }
        below[g] = wave_total + mine;
        wave_total += all;
    }
    uint32_t* row = w.row();
    if (w.lane == 0) row[w.wave] = wave_total;
    __syncthreads();
    uint32_t base = tile_counts[t];
#pragma unroll
    for (uint32_t i = 0; i < kTileWaves; i++)
        if (i < w.wave) base += row[i];
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
    {
        // (mbcnt counted the lanes below for every element position: the lane's own earlier elements of the pack are added here)
        uint32_t rank = base + below[g];
#pragma unroll
        for (uint32_t k = 0; k < C::VEC; k++)
        {
            if ((f >> (g * C::VEC + k)) & 1u)
            {
                emit(rank, g, k, i0 + g * C::PACK_STRIDE + k);
                rank++;
            }
        }
    }
}

} // namespace glu_hip
