// key_runs_kernels.hpp -- gfx950 kernels of KEY RUNS (glu_key_runs_run_ptr): the heads of the runs of equal keys in an array,
// written as an offsets array in the form the batched sort, reduce and scan take.  Not in the reference.
//
// A head is an index i with i == 0 or ((keys[i] ^ keys[i - 1]) & mask) != 0.  Three kernels, whatever the keys hold:
//   key_runs_count_kernel   tile_counts[t] = heads of tile t.  A tile is KeyRunsCfg::TILE keys: 256 threads x 4 packs of 16 bytes,
//                           laid out like a tile of scan_batch_range (wave-major, then group, then lane, then the keys of a pack),
//                           so that the order of (wave, group, lane, key) is the order of the keys.  Tiles are counted from the
//                           16-byte boundary at or below `keys`: every pack is aligned, whole packs take one 16-byte load, the packs
//                           that hold the first and the last key go key by key, and nothing outside the array is read.  The key in
//                           front of a pack comes from the lane below (a shuffle), for lane 0 from lane 63 of the group before,
//                           and from memory only for the first pack of a wave.  One ballot + popcount per key of a pack, the four
//                           wave sums through LDS, one barrier per tile (two rows of LDS in turn, as in scan_batch_range).
//   key_runs_scan_kernel    one workgroup: tile_counts scanned exclusively in place by scan_batch_range -- the tile loop that
//                           scan_batch_block_kernel runs over a long segment's partials, 4096 counts per round with a running
//                           carry -- and the total written to *num_runs.
//   key_runs_write_kernel   the flags of a tile again; the rank of a head = tile_counts[t] + the wave sums below its wave (LDS) +
//                           the heads below it in its wave (mbcnt of the ballots); offsets[rank] = i and unique_keys[rank] =
//                           keys[i] where rank < max_runs.  The same threads then fill offsets[min(R, max_runs) .. max_runs] with
//                           `count`, R read from *num_runs.
// The keys are read twice (8 B per 4-byte key); nothing waits for another workgroup: no look-back, no atomics, no arrival order.
// Both streaming kernels run a grid sized to the device and walk the tiles in a loop.
#pragma once

#include "scan_batch_kernels.hpp"

namespace glu_hip
{
constexpr int kKrThreads = kSbThreads;
constexpr int kKrWaves = kKrThreads / kW;
constexpr uint32_t kKrGroups = 4;                                                 // packs per thread and tile
constexpr uint32_t kKrScanRound = ScanCfg<uint32_t, 4, kSbThreads>::CHUNK;        // counts per round of the count scan

template<typename K>
struct KeyRunsCfg
{
    static constexpr uint32_t VEC = 16 / (uint32_t) sizeof(K);
    static constexpr uint32_t WAVE_KEYS = kW * kKrGroups * VEC;
    static constexpr uint32_t TILE = kKrWaves * WAVE_KEYS;
};

// host only: keys per tile, tiles of `count` keys from an aligned base, rounds of the count scan
inline void key_runs_plan(uint64_t count, uint32_t key_bytes, uint32_t& tile, uint32_t& tiles, uint32_t& scan_rounds)
{
    tile = key_bytes == 8 ? KeyRunsCfg<uint64_t>::TILE : KeyRunsCfg<uint32_t>::TILE;
    tiles = (uint32_t) ((count + tile - 1) / tile);
    scan_rounds = (tiles + kKrScanRound - 1) / kKrScanRound;
}

// What a call passes to its two streaming kernels.  `base` is the 16-byte boundary at or below the keys; the keys are the
// elements [lo, hi) of it (lo < VEC).
template<typename K>
struct KeyRunsArgs
{
    const K* base;
    uint64_t lo, hi;
    K mask;
    uint32_t tiles;
};

// The calling lane's keys of tile `t` and their head flags: bit g * VEC + k for key k of the lane's pack g.  Keys outside
// [lo, hi) read as 0 and are no heads.
template<typename K>
__device__ __forceinline__ uint32_t key_runs_flags(const KeyRunsArgs<K>& a, uint32_t t, uint32_t wave, uint32_t lane,
                                                   K (&x)[kKrGroups][KeyRunsCfg<K>::VEC], uint64_t& first)
{
    using C = KeyRunsCfg<K>;
    first = (uint64_t) t * C::TILE + wave * C::WAVE_KEYS + lane * C::VEC; // the lane's pack 0; pack g: + g * kW * VEC
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t g = 0; g < kKrGroups; g++)
    {
        const uint64_t v0 = first + g * kW * C::VEC;
        if (v0 >= a.lo && v0 + C::VEC <= a.hi)
        {
            const Pack<K, C::VEC> pk = *reinterpret_cast<const Pack<K, C::VEC>*>(a.base + v0);
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++) x[g][k] = pk.v[k];
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++) x[g][k] = (v0 + k >= a.lo && v0 + k < a.hi) ? a.base[v0 + k] : (K) 0;
        }
        K prev = shfl_up_t(x[g][C::VEC - 1], 1);
        if (g == 0)
        {
            if (lane == 0) prev = (v0 > a.lo && v0 < a.hi) ? a.base[v0 - 1] : (K) 0;
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
            const bool head = v >= a.lo && v < a.hi && (v == a.lo || ((x[g][k] ^ prev) & a.mask) != 0);
            flags |= (head ? 1u : 0u) << (g * C::VEC + k);
            prev = x[g][k];
        }
    }
    return flags;
}

template<typename K>
__global__ __launch_bounds__(kKrThreads) void key_runs_count_kernel(KeyRunsArgs<K> a, uint32_t* __restrict__ tile_counts)
{
    using C = KeyRunsCfg<K>;
    __shared__ uint32_t wsum[2][kKrWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t phase = 0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        K x[kKrGroups][C::VEC];
        uint64_t first;
        const uint32_t flags = key_runs_flags(a, t, wave, lane, x, first);
        uint32_t n = 0;
#pragma unroll
        for (uint32_t b = 0; b < kKrGroups * C::VEC; b++) n += (uint32_t) __popcll(__ballot((flags >> b) & 1u));
        uint32_t* row = wsum[phase & 1u];
        phase++;
        if (lane == 0) row[wave] = n;
        __syncthreads();
        if (threadIdx.x == 0)
        {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < kKrWaves; w++) sum += row[w];
            tile_counts[t] = sum;
        }
    }
}

// One workgroup.  tile_counts[0 .. tiles) becomes its exclusive scan, *num_runs the total.
__global__ __launch_bounds__(kSbThreads) void key_runs_scan_kernel(uint32_t* __restrict__ tile_counts, uint32_t tiles,
                                                                   uint32_t* __restrict__ num_runs)
{
    using T = Elem<uint32_t, 1>;
    __shared__ T wsum[2][kSbWaves];
    __shared__ uint32_t last;
    if (threadIdx.x == 0) last = tiles ? tile_counts[tiles - 1] : 0u;
    __syncthreads();
    uint32_t phase = 0;
    scan_batch_range<uint32_t, 1>(reinterpret_cast<T*>(tile_counts), tiles, zero_elem<uint32_t, 1>(), threadIdx.x, wsum, phase);
    __syncthreads(); // (the last count's scan was stored by another thread of this workgroup)
    if (threadIdx.x == 0) *num_runs = tiles ? tile_counts[tiles - 1] + last : 0u;
}

template<typename K>
__global__ __launch_bounds__(kKrThreads) void key_runs_write_kernel(KeyRunsArgs<K> a, const uint32_t* __restrict__ tile_counts,
                                                                    const uint32_t* __restrict__ num_runs, K* __restrict__ unique_keys,
                                                                    uint32_t* __restrict__ offsets, uint32_t max_runs)
{
    using C = KeyRunsCfg<K>;
    __shared__ uint32_t wsum[2][kKrWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t phase = 0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        K x[kKrGroups][C::VEC];
        uint64_t first;
        const uint32_t flags = key_runs_flags(a, t, wave, lane, x, first);
        uint32_t below[kKrGroups]; // heads of the wave in front of the lane's pack g
        uint32_t wave_total = 0;
#pragma unroll
        for (uint32_t g = 0; g < kKrGroups; g++)
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
        for (int w = 0; w < kKrWaves; w++)
            if ((uint32_t) w < wave) base += row[w];
#pragma unroll
        for (uint32_t g = 0; g < kKrGroups; g++)
        {
            uint32_t rank = base + below[g];
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++)
            {
                if ((flags >> (g * C::VEC + k)) & 1u)
                {
                    if (rank < max_runs)
                    {
                        offsets[rank] = (uint32_t) (first + g * kW * C::VEC + k - a.lo);
                        if (unique_keys) unique_keys[rank] = x[g][k];
                    }
                    rank++;
                }
            }
        }
    }
    // the entries behind the last run, offsets[max_runs] among them
    const uint32_t runs = *num_runs;
    const uint32_t count = (uint32_t) (a.hi - a.lo);
    for (uint64_t r = (uint64_t) (runs < max_runs ? runs : max_runs) + blockIdx.x * (uint64_t) kKrThreads + threadIdx.x; r <= max_runs;
         r += (uint64_t) gridDim.x * kKrThreads)
        offsets[r] = count;
}

} // namespace glu_hip
