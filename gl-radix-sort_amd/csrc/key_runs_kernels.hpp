// key_runs_kernels.hpp -- gfx950 kernels of KEY RUNS (glu_key_runs_run_ptr): the heads of the runs of equal keys in an array,
// written as an offsets array in the form the batched sort, reduce and scan take.  Not in the reference.
//
// A head is an index i with i == 0 or ((keys[i] ^ keys[i - 1]) & mask) != 0.  Key runs is a flag-and-compact operator
// (tile_compact_kernels.hpp: the tiles, the load of a pack, the count per tile, the ranks); what it adds:
//   the flags   key_runs_flags: a neighbour comparison under a mask.  The key in front of a pack comes from the lane below (a
//               shuffle), for lane 0 from lane 63 of the pack before, and from memory only for the first pack of a wave.  The keys
//               stay in registers for the write.
//   the write   offsets[rank] = i and unique_keys[rank] = keys[i] where rank < max_runs.
//   the fill    the threads of key_runs_write_kernel then fill offsets[min(R, max_runs) .. max_runs] with `count`, R read from
//               *num_runs.
// The keys are read twice (8 B per 4-byte key).
#pragma once

#include "tile_compact_kernels.hpp"

namespace glu_hip
{
constexpr uint32_t kKeyRunsPacks = 4;
template<typename K>
using KeyRunsCfg = TileCfg<sizeof(K), kKeyRunsPacks>;

// What a call passes to its two streaming kernels.
template<typename K>
struct KeyRunsArgs
{
    TileSpan<K> keys;
    K mask;
};

// The calling lane's keys of a tile (`first`: its pack 0) and their head flags.  Keys outside the array read as 0 and are no heads.
template<typename K>
__device__ __forceinline__ uint32_t key_runs_flags(const KeyRunsArgs<K>& a, uint64_t first, uint32_t lane,
                                                   K (&x)[kKeyRunsPacks][KeyRunsCfg<K>::VEC])
{
    using C = KeyRunsCfg<K>;
    const TileSpan<K>& s = a.keys;
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
    {
        const uint64_t v0 = first + g * C::PACK_STRIDE;
        tile_load_pack<C::VEC>(s, v0, [&](uint32_t k, K key, bool) { x[g][k] = key; });
        K prev = shfl_up_t(x[g][C::VEC - 1], 1);
        if (g == 0)
        {
            if (lane == 0) prev = (v0 > s.lo && v0 < s.hi) ? s.base[v0 - 1] : (K) 0;
        }
        else
        {
            const K below = shfl_t(x[g - 1][C::VEC - 1], kW - 1);
            if (lane == 0) prev = below;
        }
#pragma unroll
        for (uint32_t k = 0; k < C::VEC; k++)
        {
            const uint64_t v = v0 + k;
            const bool head = v >= s.lo && v < s.hi && (v == s.lo || ((x[g][k] ^ prev) & a.mask) != 0);
            flags |= (head ? 1u : 0u) << (g * C::VEC + k);
            prev = x[g][k];
        }
    }
    return flags;
}

template<typename K>
__global__ __launch_bounds__(kTileThreads) void key_runs_count_kernel(KeyRunsArgs<K> a, uint32_t* __restrict__ tile_counts)
{
    using C = KeyRunsCfg<K>;
    TileWalk<C> w;
    for (uint32_t t = blockIdx.x; t < a.keys.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        K x[C::PACKS][C::VEC];
        tile_count(w, t, key_runs_flags(a, w.first(t), w.lane, x), tile_counts);
    }
}

// (the second bound, eight waves per SIMD, keeps the kernel at 80 scalar registers or fewer, the most with which eight waves are
// what the device gives: DESIGN.md 4.11, "The launch bound of the write kernel", and the uint64 row of profiles/key_runs/ladder.txt)
template<typename K>
__global__ __launch_bounds__(kTileThreads, 8) void key_runs_write_kernel(KeyRunsArgs<K> a, const uint32_t* __restrict__ tile_counts,
                                                                      const uint32_t* __restrict__ num_runs, K* __restrict__ unique_keys,
                                                                      uint32_t* __restrict__ offsets, uint32_t max_runs)
{
    using C = KeyRunsCfg<K>;
    TileWalk<C> w;
    for (uint32_t t = blockIdx.x; t < a.keys.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        K x[C::PACKS][C::VEC];
        const uint32_t flags = key_runs_flags(a, w.first(t), w.lane, x);
        tile_compact(w, t, flags, a.keys, tile_counts, [&](uint32_t rank, uint32_t g, uint32_t k, uint32_t i) {
            if (rank < max_runs)
            {
                offsets[rank] = i;
                if (unique_keys) unique_keys[rank] = x[g][k];
            }
        });
    }
    // the entries behind the last run, offsets[max_runs] among them
    const uint32_t runs = *num_runs;
    const uint32_t count = (uint32_t) (a.keys.hi - a.keys.lo);
    for (uint64_t r = (uint64_t) (runs < max_runs ? runs : max_runs) + blockIdx.x * (uint64_t) kTileThreads + threadIdx.x; r <= max_runs;
         r += (uint64_t) gridDim.x * kTileThreads)
        offsets[r] = count;
}

} // namespace glu_hip
