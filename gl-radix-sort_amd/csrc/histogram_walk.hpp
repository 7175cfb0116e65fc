// histogram_walk.hpp -- the walk of the counting kernels: every tile of an array, the bin of each element by a rule, the adds with
// their skew handling.  Templates only, so that more than one translation unit can include it: histogram_kernels.hpp (its kernels
// count samples per bin) and topk_kernels.hpp (its kernels count the digits of a radix select) walk with it.
//
// The elements are read once, in whole 16-byte packs from the 16-byte boundary at or below the array, the elements in front of and
// behind the array masked (tile_span.hpp's TileSpan and tile_load_pack); a tile is THREADS x 4 packs, pack g of thread t being pack
// g * THREADS + t of the tile: the order of the elements does not matter to a count, so the lanes simply lie side by side.
// Skew (hist_add_bins): a wave whose counted samples of a tile all fall into ONE bin issues one add of their number, and holds it back
// while the next tiles fall into the same bin; otherwise every thread adds the runs of equal bins among its 16 or 8 samples, one
// add per run.  Counts are integers: the adds commute, and
// the same input gives the same bits whatever the arrival order.
#pragma once

#include <type_traits>

#include "histogram_bins.hpp"
#include "tile_compact_kernels.hpp"

namespace glu_hip
{
// A call as its streaming kernel sees it.  Rule: HistEvenInt, HistEvenFloat, HistEdges<T>, or another unit's own (a rule is what
// hist_bin_of(rule, x, lds_edges) is overloaded for).
template<typename T>
struct HistEdges
{
    const T* edges;   // bins + 1 values on the device
    uint32_t n_edges; // bins + 1
    uint32_t steps;   // hist_steps(n_edges)
};

template<typename T, typename Rule>
struct HistArgs
{
    TileSpan<T> samples; // tiles: of THIS operator's tile (hist_tile), counted from the span's base
    Rule rule;
    uint32_t bins;
    uint32_t* dst; // LDS path: partial[groups][bins]; GLOBAL path: out_counts
};

template<typename T>
__device__ __forceinline__ uint32_t hist_bin_of(const HistEvenInt& r, T x, const T*)
{
    return hist_even_int_bin(r, x);
}
template<typename T>
__device__ __forceinline__ uint32_t hist_bin_of(const HistEvenFloat& r, T x, const T*)
{
    return hist_even_float_bin(r, x);
}
// (the edges are searched where the workgroup staged them: in LDS)
template<typename T>
__device__ __forceinline__ uint32_t hist_bin_of(const HistEdges<T>& r, T x, const T* lds_edges)
{
    return hist_edges_bin(x, r.n_edges, r.steps, [&](uint32_t i) { return lds_edges[i]; });
}

// What a wave carries from tile to tile: the bin that held ALL its counted samples of the tiles before, and their number, not yet
// added (wave-uniform; lane 0 adds it).  Input that is one value costs a wave one add per call, not one per tile.
struct HistPending
{
    uint32_t bin = kHistNoBin, n = 0;
    template<typename Add>
    __device__ __forceinline__ void flush(Add add)
    {
        if (n && (threadIdx.x & 63u) == 0) add(bin, n);
        n = 0;
    }
};

// The bins of one thread's samples of a tile (kHistNoBin: not counted) into the table behind add(bin, n).  Called by whole waves.
template<uint32_t N, typename Add>
__device__ __forceinline__ void hist_add_bins(const uint32_t (&bin)[N], HistPending& pending, Add add)
{
    uint32_t mine = kHistNoBin; // the thread's first counted bin
    bool same = true;           // all its counted bins are that one
#pragma unroll
    for (uint32_t e = 0; e < N; e++)
    {
        const bool counted = bin[e] != kHistNoBin;
        same = same && (!counted || mine == kHistNoBin || bin[e] == mine);
        mine = mine == kHistNoBin ? bin[e] : mine;
    }
    const uint64_t lanes = __ballot(mine != kHistNoBin);
    if (lanes == 0) return; // (wave-uniform)
    const uint32_t first = (uint32_t) __builtin_amdgcn_readlane((int) mine, (int) __builtin_ctzll(lanes));
    if (__ballot(mine != kHistNoBin && (!same || mine != first)) == 0) // (wave-uniform) one bin holds all the wave counts
    {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t e = 0; e < N; e++) total += (uint32_t) __popcll(__ballot(bin[e] != kHistNoBin));
        if (first != pending.bin) pending.flush(add);
        pending.bin = first;
        pending.n += total; // (below 2^32: a call counts fewer samples than that)
        return;
    }
    uint32_t cur = kHistNoBin, n = 0; // the run of equal bins so far
#pragma unroll
    for (uint32_t e = 0; e < N; e++)
    {
        if (bin[e] != cur)
        {
            if (n) add(cur, n);
            cur = bin[e];
            n = 0;
        }
        n += bin[e] != kHistNoBin ? 1u : 0u;
    }
    if (n) add(cur, n);
}

// every tile g, g + gridDim.x, ... of the samples: the bins of the calling thread's packs, added.  The packs of the next tile are
// loaded before the bins of this one are added: their latency lies under the adds.
template<typename T, uint32_t THREADS, typename Rule, typename Add>
__device__ __forceinline__ void hist_walk(const HistArgs<T, Rule>& a, const T* lds_edges, Add add)
{
    constexpr uint32_t VEC = 16 / sizeof(T), N = kHistPacks * VEC, TILE = THREADS * N;
    static_assert(TILE == hist_tile(sizeof(T), std::is_same<Rule, HistEdges<T>>::value ? HIST_EDGES : HIST_EVEN), "the plan's tile");
    static_assert(N <= 32, "a thread's samples inside the array are the bits of one word");
    // the calling thread's samples of tile t, and which of them lie inside the array
    auto load = [&](uint32_t t, T (&x)[N], uint32_t& inside) {
        const uint64_t first = (uint64_t) t * TILE + threadIdx.x * VEC;
        inside = 0;
#pragma unroll
        for (uint32_t g = 0; g < kHistPacks; g++)
            tile_load_pack<VEC>(a.samples, first + (uint64_t) g * THREADS * VEC, [&](uint32_t k, T v, bool in) {
                x[g * VEC + k] = v;
                inside |= (in ? 1u : 0u) << (g * VEC + k);
            });
    };
    HistPending pending;
    T x[N];
    uint32_t inside = 0;
    uint32_t t = blockIdx.x;
    if (t < a.samples.tiles) load(t, x, inside);
    while (t < a.samples.tiles) // (workgroup-uniform)
    {
        T next[N];
        uint32_t next_inside = 0;
        const uint32_t tn = t + gridDim.x; // (tiles + groups < 2^32: tiles <= 2^20 + 1)
        if (tn < a.samples.tiles) load(tn, next, next_inside);
        uint32_t bin[N];
#pragma unroll
        for (uint32_t e = 0; e < N; e++) bin[e] = (inside >> e) & 1u ? hist_bin_of(a.rule, x[e], lds_edges) : kHistNoBin;
        hist_add_bins<N>(bin, pending, add);
#pragma unroll
        for (uint32_t e = 0; e < N; e++) x[e] = next[e];
        inside = next_inside;
        t = tn;
    }
    pending.flush(add);
}

} // namespace glu_hip
