// sorted_search_kernels.hpp -- gfx950 kernels of SORTED SEARCH (glu_sorted_search_run_ptr): the lower and the upper bound of many
// needles in a sorted haystack, numpy.searchsorted on the device.  Not in the reference.
//
// With enc = the sort's KeyCodec::encode (radix_sort_kernels.hpp), which maps all six key types to unsigned keys in the order the
// sort produces:  lower[j] = #{i : enc(hay[i]) < enc(needles[j])},  upper[j] = #{i : enc(hay[i]) <= enc(needles[j])}.
//
// Every search here is the same loop: the bound is built bit by bit from the top (pos += step where the key at pos + step - 1
// passes), with a trip count that follows from the LENGTH searched and not from the keys, so that a wave never diverges, and with
// every probe index clamped to the range searched, so that an unsorted haystack gives a wrong position and never a read outside.
//   direct    sorted_search_direct_kernel: the loop over the whole haystack in global memory, ceil(log2(hay_count + 1)) probes, one
//             needle per lane slot.
//   index     sorted_search_index_kernel: level k >= 1 of the index is len_k = hay_count >> (k * log2 F) encoded keys,
//             level_k[t] = enc(hay[(t + 1) * F^k - 1]), F = 128 / sizeof(key) keys to the 128-byte line.  Every level is a strided
//             sample of the haystack itself: one kernel writes them all, a thread per entry.
//   indexed   sorted_search_kernel: the top level (at most 32 KiB) is copied to LDS once per workgroup and searched there; then
//             one NODE per level below: with p the bound in level k + 1, the bound in level k lies in [p * F, p * F + F - 1]
//             (entry p of level k + 1 is the last key of that node and does not pass, or the node is the short one at the end), so
//             log2 F probes inside one line give it.  Level 0 is the haystack, encoded on load.
// The indexed search walks the needles as the tiles of tile_span.hpp (16-byte packs from the boundary at or below the array); the
// several needles of a thread advance side by side: step by step, never needle by needle, so that their loads are in flight
// together.  No atomics, no look-back, nothing waits for another workgroup.
#pragma once

#include "radix_sort_kernels.hpp"
#include "tile_compact_kernels.hpp"

namespace glu_hip
{
constexpr uint32_t kSearchPacks = 2;         // 16-byte packs of needles per thread and tile
constexpr uint32_t kSearchMaxLevels = 8;     // level 0 (the haystack) .. 7: TOP_ENTRIES = F = 16 and 2^32 - 1 keys take 7
constexpr uint32_t kSearchLdsBytes = 32768;  // the top level in LDS: 8192 4-byte or 4096 8-byte entries at the most
template<typename K>
using SearchCfg = TileCfg<sizeof(K), kSearchPacks>;

constexpr uint32_t search_fanout(uint32_t key_bytes) { return 128u / key_bytes; }
constexpr uint32_t search_log2_fanout(uint32_t key_bytes) { return key_bytes == 4 ? 5u : 4u; }
constexpr uint32_t search_lds_entries(uint32_t key_bytes) { return kSearchLdsBytes / key_bytes; }

enum
{
    SEARCH_LOWER = 1,
    SEARCH_UPPER = 2,
    SEARCH_BOTH = 3
};

// The haystack and its index as the kernels see them: level[0] = the haystack (raw keys), level[k] = the encoded samples.
template<typename K>
struct SearchLevels
{
    const K* level[kSearchMaxLevels];
    uint32_t len[kSearchMaxLevels];
    uint32_t levels; // L: the top level; 0 = no index
    uint32_t xf;     // KeyTransform of the key type
};

// trips of the bound loop over `len` keys: the bound is one of 0 .. len
__host__ __device__ inline uint32_t search_steps(uint32_t len) { return len ? 32u - (uint32_t) __builtin_clz(len) : 0u; }

// does a key of the haystack lie in front of the bound of x?  (lower: the keys below x; upper: the keys not above it)
template<bool UPPER, typename K>
__device__ __forceinline__ bool search_passes(K key, K x)
{
    return UPPER ? key <= x : key < x;
}

// The needles of the calling lane in tile t, encoded; bound(x, lower, upper) for all of them at once; the results stored.
// BOUNDS: SEARCH_LOWER, SEARCH_UPPER or SEARCH_BOTH.  N chains per bound.
template<typename K, int BOUNDS, typename Search>
__device__ __forceinline__ void search_tile(const TileSpan<K>& needles, uint64_t first, const KeyCodec<K, true>& codec,
                                            uint32_t* __restrict__ out_lower, uint32_t* __restrict__ out_upper, Search search)
{
    using C = SearchCfg<K>;
    constexpr uint32_t N = C::PACKS * C::VEC;
    K x[N];
    uint32_t inside = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
        tile_load_pack<C::VEC>(needles, first + g * C::PACK_STRIDE, [&](uint32_t k, K key, bool in) {
            x[g * C::VEC + k] = codec.encode(key);
            inside |= (in ? 1u : 0u) << (g * C::VEC + k);
        });
    uint32_t lower[N], upper[N];
    search(x, lower, upper);
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
#pragma unroll
        for (uint32_t k = 0; k < C::VEC; k++)
            if ((inside >> (g * C::VEC + k)) & 1u)
            {
                const uint64_t j = first + g * C::PACK_STRIDE + k - needles.lo; // the needle as an element of its array
                if (BOUNDS & SEARCH_LOWER) out_lower[j] = lower[g * C::VEC + k];
                if (BOUNDS & SEARCH_UPPER) out_upper[j] = upper[g * C::VEC + k];
            }
}

// pos[e] = base[e] + the bound of x[e] among the len[e] keys from base[e] on: `steps` trips (2^steps > every len), every needle
// of the thread in every trip.  key_at(i, any): the encoded key i, read only where any (a range of no keys has none to read).
template<bool UPPER, uint32_t N, typename K, typename KeyAt>
__device__ __forceinline__ void search_range(const K (&x)[N], const uint32_t (&base)[N], const uint32_t (&len)[N], uint32_t steps,
                                             uint32_t (&pos)[N], KeyAt key_at)
{
#pragma unroll
    for (uint32_t e = 0; e < N; e++) pos[e] = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1) // (kernel-uniform)
    {
#pragma unroll
        for (uint32_t e = 0; e < N; e++)
        {
            const uint32_t next = pos[e] + step;
            const uint32_t probe = (next < len[e] ? next : len[e]); // clamped: 1 <= probe <= len where len > 0
            const K key = key_at(base[e] + (probe ? probe - 1u : 0u), len[e] != 0u);
            pos[e] = (next <= len[e] && search_passes<UPPER>(key, x[e])) ? next : pos[e];
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < N; e++) pos[e] += base[e];
}

// DIRECT: every needle against the whole haystack, one needle per lane slot: few needles spread over as many waves as there are,
// and many needles of a short haystack find it in the caches.  The needles are read and the bounds written 4 or 8 bytes a lane,
// side by side; workgroup b takes the needles [b * 256, b * 256 + 256) and then those a grid further.
template<typename K, int BOUNDS>
__global__ __launch_bounds__(kTileThreads) void sorted_search_direct_kernel(const K* __restrict__ hay, uint32_t hay_count, uint32_t xf,
                                                                            const K* __restrict__ needles, uint32_t needle_count,
                                                                            uint32_t* __restrict__ out_lower, uint32_t* __restrict__ out_upper)
{
    const KeyCodec<K, true> codec(xf);
    const uint32_t steps = search_steps(hay_count);
    const uint32_t base[1] = {0u}, len[1] = {hay_count};
    auto key_at = [&](uint32_t i, bool any) { return any ? codec.encode(hay[i]) : (K) 0; };
    for (uint64_t j = (uint64_t) blockIdx.x * kTileThreads + threadIdx.x; j < needle_count; j += (uint64_t) gridDim.x * kTileThreads)
    {
        const K x[1] = {codec.encode(needles[j])};
        uint32_t pos[1];
        if (BOUNDS & SEARCH_LOWER)
        {
            search_range<false>(x, base, len, steps, pos, key_at);
            out_lower[j] = pos[0];
        }
        if (BOUNDS & SEARCH_UPPER)
        {
            search_range<true>(x, base, len, steps, pos, key_at);
            out_upper[j] = pos[0];
        }
    }
}

// The index: entry t of level k = enc(hay[(t + 1) * F^k - 1]) for k = 1 .. levels, a thread per entry of all the levels.
template<typename K>
struct SearchIndexArgs
{
    const K* hay;
    K* level[kSearchMaxLevels]; // (level[0] is not used)
    uint32_t len[kSearchMaxLevels];
    uint32_t levels, xf;
    uint32_t entries; // len[1] + .. + len[levels]
};

template<typename K>
__global__ __launch_bounds__(kTileThreads) void sorted_search_index_kernel(SearchIndexArgs<K> a)
{
    constexpr uint32_t LOG_F = search_log2_fanout(sizeof(K));
    const KeyCodec<K, true> codec(a.xf);
    uint32_t t = blockIdx.x * kTileThreads + threadIdx.x;
    if (t >= a.entries) return;
    uint32_t k = 1;
    while (k < a.levels && t >= a.len[k]) t -= a.len[k++]; // (at most six trips; entries is the sum, so t < len[k] at the end)
    if (t >= a.len[k]) return;
    // (t + 1) * F^k <= len[k] * F^k <= hay_count: the sample lies inside the haystack whatever it holds
    a.level[k][t] = codec.encode(a.hay[(((uint64_t) t + 1) << (k * LOG_F)) - 1]);
}

// INDEXED: the top level in LDS, then one node per level.
template<typename K, int BOUNDS>
__global__ __launch_bounds__(kTileThreads) void sorted_search_kernel(SearchLevels<K> s, TileSpan<K> needles, uint32_t* __restrict__ out_lower,
                                                                     uint32_t* __restrict__ out_upper)
{
    using C = SearchCfg<K>;
    constexpr uint32_t N = C::PACKS * C::VEC, F = search_fanout(sizeof(K)), LOG_F = search_log2_fanout(sizeof(K));
    constexpr uint32_t TABLE_VEC = 16 / sizeof(K);
    __shared__ Pack<K, TABLE_VEC> table_packs[kSearchLdsBytes / 16];
    const K* table = &table_packs[0].v[0];
    const KeyCodec<K, true> codec(s.xf);
    const uint32_t L = s.levels, top_len = s.len[L]; // (the host launches this kernel with 1 <= L and top_len <= the LDS entries)
    {
        // whole 16-byte packs: a level's base is aligned to 128 bytes and its room is a multiple of 128 bytes
        const Pack<K, TABLE_VEC>* src = reinterpret_cast<const Pack<K, TABLE_VEC>*>(s.level[L]);
        const uint32_t packs = (top_len + TABLE_VEC - 1) / TABLE_VEC;
        for (uint32_t i = threadIdx.x; i < packs && i < kSearchLdsBytes / 16; i += kTileThreads) table_packs[i] = src[i];
    }
    __syncthreads();
    const uint32_t top_steps = search_steps(top_len);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    auto descend = [&](auto upper_tag, const K(&x)[N], uint32_t(&p)[N]) {
        constexpr bool UPPER = decltype(upper_tag)::value;
        uint32_t base[N], len[N];
#pragma unroll
        for (uint32_t e = 0; e < N; e++) base[e] = 0, len[e] = top_len;
        search_range<UPPER>(x, base, len, top_steps, p, [&](uint32_t i, bool) { return table[i]; });
        for (uint32_t k = L - 1; k >= 1; k--) // (kernel-uniform)
        {
            const K* lvl = s.level[k];
            const uint32_t n = s.len[k];
#pragma unroll
            for (uint32_t e = 0; e < N; e++)
            {
                const uint32_t b = p[e] << LOG_F; // p <= len[k + 1] = n >> LOG_F: b <= n
                const uint32_t rest = n - (b < n ? b : n);
                base[e] = b < n ? b : n;
                len[e] = rest < F - 1 ? rest : F - 1;
            }
            search_range<UPPER>(x, base, len, LOG_F, p, [&](uint32_t i, bool any) { return any ? lvl[i] : (K) 0; });
        }
        {
            const K* hay = s.level[0];
            const uint32_t n = s.len[0];
#pragma unroll
            for (uint32_t e = 0; e < N; e++)
            {
                const uint32_t b = p[e] << LOG_F;
                const uint32_t rest = n - (b < n ? b : n);
                base[e] = b < n ? b : n;
                len[e] = rest < F - 1 ? rest : F - 1;
            }
            search_range<UPPER>(x, base, len, LOG_F, p, [&](uint32_t i, bool any) { return any ? codec.encode(hay[i]) : (K) 0; });
        }
    };

    for (uint32_t t = blockIdx.x; t < needles.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        const uint64_t first = (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC;
        search_tile<K, BOUNDS>(needles, first, codec, out_lower, out_upper, [&](const K(&x)[N], uint32_t(&lower)[N], uint32_t(&upper)[N]) {
            if (BOUNDS & SEARCH_LOWER) descend(std::false_type(), x, lower);
            if (BOUNDS & SEARCH_UPPER) descend(std::true_type(), x, upper);
        });
    }
}

} // namespace glu_hip
